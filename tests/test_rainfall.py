"""Rainfall footprints (tropical_cyclone_risk_amd/rainfall.py, csrc/tcr_rainfall.hip): storm-total rain and peak rain rate of
every storm at every site from the R-CLIPER profile.  CPU tests pin the NumPy restatement (tests/rainfall_numpy.py) to hand
values, to a closed-form total and to the record weights, and check the argument handling and the C struct layout; GPU tests
(`-m gpu`) check the kernels against the restatement, and the order guarantee of the summing scan bit for bit."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest

from tests import rainfall_numpy as RN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DT = 3600.0
KT = 1852.0 / 3600.0                        # m/s per knot
THR_TOTAL = np.array([5.0, 10.0, 25.0, 50.0, 75.0, 100.0, 150.0, 200.0, 300.0])           # mm
THR_PEAK = np.array([0.5, 1.0, 2.0, 4.0, 6.0, 8.0, 10.0, 12.0])                           # mm/h
KEY = {'total': 'site_total', 'peak-rate': 'site_peak_rate'}


# ------------------------------------------------------------------------------------------------------------------ CPU
def _terms(v_kt):
    """T0, Tm (inches/day), rm, re (km) of the default coefficients at v_kt knots, by scalar arithmetic."""
    u = 1.0 + (v_kt - 35.0) / 33.0
    return -1.10 + 3.96 * u, -1.60 + 4.80 * u, 64.5 - 13.0 * u, 150.0 - 16.0 * u


def test_profile_by_hand():
    mmh = 25.4 / 24.0
    for v_kt in (35.0, 64.0, 100.0, 155.0):
        t0, tm, rm, re = _terms(v_kt)
        v = v_kt * KT
        assert math.isclose(float(RN.rate(0.0, v)), t0 * mmh, rel_tol=1e-13)
        assert math.isclose(float(RN.rate(rm, v)), tm * mmh, rel_tol=1e-13)                           # the outer branch at rm
        assert math.isclose(float(RN.rate(np.nextafter(rm, 0.0), v)), tm * mmh, rel_tol=1e-12)        # the inner branch below it
        assert math.isclose(float(RN.rate(rm + re, v)), tm * mmh / math.e, rel_tol=1e-13)
        assert math.isclose(float(RN.rate(rm / 2, v)), (t0 + tm) / 2 * mmh, rel_tol=1e-13)
    # units, for one vmax: 50 m/s = 97.19 kt, U = 2.8846, Tm = 12.246 inches/day = 12.96 mm/h at rm = 27.0 km
    kt = 50.0 * 3600.0 / 1852.0
    u = 1.0 + (kt - 35.0) / 33.0
    assert math.isclose(kt, 97.192, rel_tol=1e-5) and math.isclose(u, 2.88461, rel_tol=1e-5)
    tm, rm = -1.60 + 4.80 * u, 64.5 - 13.0 * u
    assert math.isclose(rm, 27.0, rel_tol=1e-3) and math.isclose(tm * 25.4 / 24.0, 12.96, rel_tol=1e-3)
    assert math.isclose(float(RN.rate(rm, 50.0)), tm * 25.4 / 24.0, rel_tol=1e-13)
    # the clamp: a depression rains like 35 kt, anything above 155 kt like 155 kt
    for r in (0.0, 10.0, 60.0, 200.0, 499.0):
        lo, hi = _terms(35.0), _terms(155.0)
        for v, (t0, tm, rm, re) in ((0.0, lo), (-3.0, lo), (10.0, lo), (200.0 * KT, hi), (1e4, hi)):
            want = max(t0 + (tm - t0) * r / rm if r < rm else tm * math.exp(-(r - rm) / re), 0.0) * mmh
            assert math.isclose(float(RN.rate(r, v)), want, rel_tol=1e-14), (r, v)
        assert math.isclose(float(RN.rate(r, 0.0)), float(RN.rate(r, 35.0 * KT)), rel_tol=1e-13)
        assert math.isclose(float(RN.rate(r, 200.0 * KT)), float(RN.rate(r, 155.0 * KT)), rel_tol=1e-12)
    # T0 < 0: no rain at the centre, never a negative rate
    a = (-10.0, -1.60, 64.5, 150.0)
    t0 = -10.0 + 3.96 * (1.0 + (50.0 - 35.0) / 33.0)
    assert t0 < 0
    assert float(RN.rate(0.0, 50.0 * KT, a=a)) == 0.0
    rr = RN.rate(np.linspace(0.0, 500.0, 2001), 50.0 * KT, a=a)
    assert (rr >= 0).all() and (rr[:50] == 0).all() and rr.max() > 5.0


def _equator_track(c_kmh, n_t, vmax):
    """One storm on the equator moving east at c km/h, hourly samples."""
    lon = 200.0 + np.rad2deg(c_kmh * np.arange(n_t) / RN.EARTH_R_KM)
    return lon[None, :], np.zeros((1, n_t)), np.full((1, n_t), vmax)


def test_closed_form_total_of_a_straight_track():
    c, n_t, vmax, r_out = 20.0, 48, 40.0, 300.0
    lon, lat, v = _equator_track(c, n_t, vmax)
    x_site = 23.37 * c                                                  # km along the track: between two samples
    assert x_site > r_out + c and (n_t - 1) * c - x_site > r_out + c    # the track passes r_out on both sides
    slon = np.array([200.0 + np.rad2deg(x_site / RN.EARTH_R_KM)])
    t0, tm, rm, re = (float(x) * RN.MMH if i < 2 else float(x) for i, x in enumerate(RN.profile_terms(vmax)))
    assert 0 < t0 < tm and rm < r_out
    exact = (2.0 / c) * ((t0 + tm) / 2 * rm + tm * re * (1.0 - math.exp(-(r_out - rm) / re)))
    L = c * max(abs(tm - t0) / rm, tm / re)                             # Lipschitz constant of the rate in time (mm/h per h)
    T = 2.0 * r_out / c
    err = {}
    for sub in (1, 4, 16):
        h = DT / 3600.0 / sub
        val, n_band = RN.site_values(RN.records(lon, lat, v, DT, sub), slon, np.array([0.0]), r_out)
        assert n_band == 0
        err[sub] = abs(float(val[0, 0]) - exact)
        assert err[sub] <= L * h * T / 4 + 2 * h * tm, (sub, err[sub], exact)
    assert err[16] < err[1]
    assert 100.0 < exact < 400.0                                        # a plausible storm total in mm


def test_record_weights_and_track_cut():
    h = DT / 3600.0
    lon, lat, v = np.array([[280.0, 280.2]]), np.array([[20.0, 20.1]]), np.array([[30.0, 32.0]])
    assert RN.records(lon, lat, v, DT, 1)[0][3].tolist() == [h / 2, h / 2]
    lon, lat, v = np.array([[280.0, 280.2, 280.4]]), np.array([[20.0, 20.1, 20.2]]), np.array([[30.0, 32.0, 36.0]])
    rec = RN.records(lon, lat, v, DT, 2)[0]
    assert rec[3].tolist() == [h / 4, h / 2, h / 2, h / 2, h / 4]       # [h'/2, h', h', h', h'/2] with h' = h / 2
    assert np.allclose(rec[0], [280.0, 280.1, 280.2, 280.3, 280.4]) and np.allclose(rec[2], [30, 31, 32, 34, 36])
    assert math.isclose(rec[3].sum(), 2 * h)                            # the weights add up to the track's duration
    # a NaN in vmax at sample k: samples 0 .. k - 1 only, whatever follows
    lon = 280.0 + 0.2 * np.arange(8.0)[None, :]
    lat, v = np.full((1, 8), 20.0), np.full((1, 8), 30.0)
    for k in range(8):
        vk = v.copy()
        vk[0, k] = np.nan
        assert RN.track_length(lon, lat, vk).tolist() == [k]
        rec = RN.records(lon, lat, vk, DT, 3)[0]
        if k < 2:
            assert rec is None
        else:
            assert rec.shape == (4, (k - 1) * 3 + 1) and rec[0][-1] == lon[0, k - 1]
            assert math.isclose(rec[3].sum(), (k - 1) * h)
    # a site at a sample of a 2-sample track: both records inside, half weights
    lon, lat, v = np.array([[280.0, 280.2]]), np.array([[20.0, 20.0]]), np.array([[40.0, 40.0]])
    val, _ = RN.site_values(RN.records(lon, lat, v, DT, 1), [280.0], [20.0], 500.0)
    r1 = float(RN.haversine_km(280.0, 20.0, 280.2, 20.0))
    assert math.isclose(val[0, 0], h / 2 * float(RN.rate(0.0, 40.0)) + h / 2 * float(RN.rate(r1, 40.0)), rel_tol=1e-14)
    pk, _ = RN.site_values(RN.records(lon, lat, v, DT, 1), [280.0], [20.0], 500.0, 'peak-rate')
    assert math.isclose(pk[0, 0], max(float(RN.rate(0.0, 40.0)), float(RN.rate(r1, 40.0))), rel_tol=1e-14)
    far, _ = RN.site_values(RN.records(lon, lat, v, DT, 1), [100.0], [-20.0], 500.0)
    assert np.isnan(far[0, 0])


def test_substeps_across_the_dateline():
    for lon_pair, want_d in (((179.5, -179.5), 1.0), ((359.8, 0.2), 0.4), ((-179.5, 179.5), -1.0)):
        lon = np.array([list(lon_pair)])
        lat, v = np.array([[10.0, 11.0]]), np.array([[30.0, 40.0]])
        rec = RN.records(lon, lat, v, DT, 4)[0]
        d = lon_pair[1] - lon_pair[0]
        d = d - 360.0 * np.floor((d + 180.0) / 360.0)
        assert math.isclose(d, want_d, rel_tol=1e-12)
        assert rec.shape == (4, 5)
        # the sub-samples step the short way round; the last one is the sample itself, in its own convention
        assert np.allclose(rec[0][:4], lon_pair[0] + d * np.array([0, 0.25, 0.5, 0.75]), rtol=0, atol=1e-12)
        assert rec[0][4] == lon_pair[1]
        assert np.allclose(rec[1], [10.0, 10.25, 10.5, 10.75, 11.0]) and np.allclose(rec[2], [30, 32.5, 35, 37.5, 40])
        # the midpoint is next to both samples, not on the other side of the globe
        assert float(RN.haversine_km(lon_pair[0], 10.0, rec[0][2], rec[1][2])) < 100.0
        val, _ = RN.site_values([rec], [lon_pair[0]], [10.0], 200.0)
        assert val[0, 0] > 0 and math.isclose(rec[3].sum(), 1.0)


def test_rain_struct_layout_matches_header():
    from tropical_cyclone_risk_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tcrisk_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n",'
           'sizeof(tcr_rain_params),offsetof(tcr_rain_params, dt_s),offsetof(tcr_rain_params, r_out_km),'
           'offsetof(tcr_rain_params, v_lo_kt),offsetof(tcr_rain_params, v_hi_kt),offsetof(tcr_rain_params, a),'
           'offsetof(tcr_rain_params, b),offsetof(tcr_rain_params, substeps),offsetof(tcr_rain_params, stat),'
           'TCR_RAIN_TOTAL,TCR_RAIN_PEAK_RATE);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'sz.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 'sz')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    P = _lib.RainParams
    assert sizes == [ctypes.sizeof(P), P.dt_s.offset, P.r_out_km.offset, P.v_lo_kt.offset, P.v_hi_kt.offset, P.a.offset, P.b.offset,
                     P.substeps.offset, P.stat.offset, _lib.RAIN_TOTAL, _lib.RAIN_PEAK_RATE]
    assert P.a.size == 32 and P.b.size == 32


def test_rainfall_symbols_exported_and_abi_version_unchanged(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_rainfall_dev', 'tcr_rainfall_host', 'tcr_rainfall_pairs'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    L.tcr_abi_version.restype = ctypes.c_int
    assert L.tcr_abi_version() == 7 and _lib.TCR_ABI_VERSION == 7


def test_argument_errors_before_any_device_work(monkeypatch):
    from tropical_cyclone_risk_amd import _lib, rainfall

    def no_library():
        raise AssertionError('the library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', no_library)
    rng = np.random.default_rng(0)
    lon, lat, v = 280 + rng.random((3, 5)), 20 + rng.random((3, 5)), 30 + rng.random((3, 5))
    g = np.zeros(3, np.int64)
    base = dict(lon=lon, lat=lat, vmax=v, groups=g, site_lon=np.array([280.0]), site_lat=np.array([20.0]), dt_s=DT)
    a0, b0 = rainfall.DEFAULT_COEFFICIENTS
    u_hi = 1.0 + (155.0 - 35.0) / 33.0
    bad = [dict(stat='sum'), dict(stat=0), dict(stat='peak-rate'),                     # peak-rate without thresholds
           dict(substeps=0), dict(substeps=65), dict(substeps=1.5), dict(substeps=True),
           dict(r_out_km=0.0), dict(r_out_km=2000.5), dict(r_out_km=np.nan), dict(dt_s=0.0), dict(dt_s=np.inf), dict(dt_s=-1.0),
           dict(thresholds=np.array([20.0, 10.0])), dict(thresholds=np.arange(65.0)), dict(thresholds=np.array([])),
           dict(thresholds=np.array([10.0, np.inf])),
           dict(coefficients=(a0, (3.96, 4.80, -64.5 / u_hi, -16.0))),                  # rm = 0 at v_hi_kt
           dict(coefficients=(a0, (3.96, 4.80, -14.0, -16.0))),                         # rm < 0 at v_hi_kt
           dict(v_hi_kt=170.0),                                                          # the defaults give rm < 0 at 170 kt
           dict(coefficients=(a0, (3.96, 4.80, -13.0, -40.0))),                         # re < 0 at v_hi_kt
           dict(coefficients=((-1.10, -6.0, 64.5, 150.0), b0)),                         # Tm < 0 at v_lo_kt
           dict(coefficients=((np.nan, -1.60, 64.5, 150.0), b0)), dict(coefficients=(a0, b0[:3])), dict(coefficients=(a0,)),
           dict(v_lo_kt=100.0, v_hi_kt=90.0), dict(v_lo_kt=0.0), dict(v_lo_kt=-5.0), dict(v_hi_kt=np.inf),
           dict(vmax=v[:, :4]), dict(groups=np.zeros(2, np.int64)), dict(groups=np.array([0, -1, 0])),
           dict(site_lat=np.array([np.nan])), dict(site_lon=np.array([1.0, 2.0])), dict(groups=np.array([0, 1, 2]), n_groups=2),
           dict(n_groups=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            rainfall.site_rain(**dict(base, **kw))
    # good arguments do reach the library
    with pytest.raises(AssertionError, match='the library was touched'):
        rainfall.site_rain(**base)
    with pytest.raises(AssertionError, match='the library was touched'):
        rainfall.site_rain(**dict(base, stat='peak-rate', thresholds=THR_PEAK, coefficients=((-10.0, -1.60, 64.5, 150.0), b0)))


def test_cli_arguments():
    from tropical_cyclone_risk_amd import analysis, rainfall
    a = rainfall.parse_args(['x.nc', '--site=-80.19,25.76', '--grid', '270:271:0.5,20:21:1', '--r-out-km', '300', '--substeps', '4',
                             '--thresholds', '20:60:10'])
    assert a.stat == 'total' and a.r_out_km == 300.0 and a.substeps == 4 and a.out == 'rain.npz'
    assert np.array_equal(a.thresholds, [20, 30, 40, 50, 60])
    assert analysis.collect_sites(a)[0].size == 7
    b = rainfall.parse_args(['x.nc', 'y.nc', '--site', '1,2'])
    assert b.tracks == ['x.nc', 'y.nc'] and b.stat == 'total' and b.r_out_km == 500.0 and b.substeps == 1
    assert np.array_equal(b.thresholds, rainfall.DEFAULT_RAIN_THRESHOLDS)
    assert np.array_equal(rainfall.DEFAULT_RAIN_THRESHOLDS, [25, 50, 75, 100, 150, 200, 250, 300, 400, 500])
    c = rainfall.parse_args(['x.nc', '--site', '1,2', '--stat', 'peak-rate', '--thresholds', '2:10:2', '--out', 'p.npz'])
    assert c.stat == 'peak-rate' and np.array_equal(c.thresholds, [2, 4, 6, 8, 10]) and c.out == 'p.npz'
    for argv in (['x.nc'], ['x.nc', '--site', '1,2', '--stat', 'peak-rate'], ['x.nc', '--site', '1,2', '--stat', 'mean']):
        with pytest.raises(SystemExit):
            rainfall.parse_args(argv)


# ------------------------------------------------------------------------------------------------------------------ GPU
N_SPECIAL = 8       # storms 0 .. 7 of _stress_tracks, see there
FAR = 7             # the storm no site is near


def _stress_tracks(rng, n_trk=140, n_t=48):
    """Random walks of plausible storms in one wide basin around the dateline (160 E .. 145 W, both hemispheres, both longitude
    conventions), so that a tile of sites has a cap small enough for culling to happen.  NaN tails in any of the three planes.
    Storms 0, 1, 2: 0, 1 and 2 valid samples; 3, 4: 33 and 34 samples (at substeps 1 the last segment holds 1 or 2 records,
    at substeps 3 storm 3 has 97 = 3 x 32 + 1); 5: 12 samples (34 records at substeps 3); 6: runs pole-ward to 60 N; 7 (FAR): off
    Africa, farther than any r_out from every site."""
    lon0 = np.concatenate([rng.uniform(160, 215, 100), rng.uniform(176, 184, 40)])[:n_trk]
    lat0 = np.concatenate([rng.uniform(5, 35, 60), rng.uniform(-30, -5, 40), rng.uniform(-3, 3, 40)])[:n_trk]
    step_lon = rng.normal(-0.15, 0.25, (n_trk, 1)) + rng.normal(0, 0.05, (n_trk, n_t))
    step_lat = rng.normal(0.1, 0.15, (n_trk, 1)) + rng.normal(0, 0.05, (n_trk, n_t))
    lon0[6], lat0[6], step_lat[6] = 190.0, 38.0, 0.5
    lon0[FAR], lat0[FAR] = 20.0, -10.0
    lon = lon0[:, None] + np.cumsum(step_lon, axis=1) - step_lon[:, :1]
    lat = np.clip(lat0[:, None] + np.cumsum(step_lat, axis=1) - step_lat[:, :1], -60, 60)
    conv = rng.random(n_trk) < 0.5
    conv[FAR] = False
    lon[conv] = np.where(lon[conv] > 180, lon[conv] - 360, lon[conv])          # [-180, 180) for half of them
    v = np.clip(25 + np.cumsum(rng.normal(0.3, 1.5, (n_trk, n_t)), axis=1), -2, 85)       # below 35 kt and above 155 kt too
    end = rng.integers(2, n_t + 1, n_trk)
    end[:N_SPECIAL] = [0, 1, 2, 33, 34, 12, n_t, n_t]
    end[N_SPECIAL:40] = n_t
    planes = [lon, lat, v]
    for i in range(n_trk):
        if end[i] < n_t:
            planes[rng.integers(0, 3)][i, end[i]] = np.nan                 # a NaN in one plane ends the track ...
            if rng.random() < 0.5:
                for p in planes:                                          # ... and the reference writes NaN tails
                    p[i, end[i]:] = np.nan
    assert RN.track_length(lon, lat, v)[:N_SPECIAL].tolist() == [0, 1, 2, 33, 34, 12, n_t, n_t]
    return lon, lat, v


def _stress_sites(rng, lon, lat, v, r_out):
    """70 sites (not a multiple of 64): one exactly at the second sample of storm 2, one pole-ward of storm 6's end, six at rm and rm + re from a
    sample, 50 at random distances from samples, 12 anywhere in the basin.  None is near storm FAR."""
    live = np.argwhere(np.isfinite(lon) & np.isfinite(lat) & np.isfinite(v) & (np.arange(lon.shape[0]) != FAR)[:, None])
    pick = live[rng.choice(len(live), 57, replace=False)]
    cl, ca, cv = (p[pick[:, 0], pick[:, 1]] for p in (lon, lat, v))
    _, _, rm, re = RN.profile_terms(cv[1:7])
    kl, ka = RN.direct(cl[1:7], ca[1:7], np.where(np.arange(6) < 3, rm, rm + re), rng.uniform(0, 6.3, 6))
    nl_, na_ = RN.direct(cl[7:], ca[7:], rng.uniform(5, 1.3 * r_out, 50), rng.uniform(0, 6.3, 50))
    nl_[:10] += 360.0
    nl_[10:20] -= 360.0
    slon = np.concatenate([[lon[2, 1]], [lon[6, -1]], kl, nl_, rng.uniform(160, 215, 12)])
    slat = np.concatenate([[lat[2, 1]], [lat[6, -1] + 3.0], ka, na_, rng.uniform(-35, 45, 12)])
    assert slon.size == 70 and slat[1] > 60.0
    assert RN.haversine_km(lon[FAR, 0], lat[FAR, 0], slon, slat).min() > 5000.0
    return slon, slat


def _groups(rng, n_trk):
    groups = np.zeros(n_trk, np.int64)
    groups[rng.choice(n_trk, 40, replace=False)] = 2
    groups[7] = 3
    rng.shuffle(groups)
    return groups, 5                                                      # groups 1 and 4 (at least) empty


def _check(res, stat, recs, groups, n_groups, slon, slat, r_out, thr, **prof):
    """The inputs have no pair in the r_out band and no value within the tolerance of a threshold (asserted here, on the CPU
    side); then site values within the tolerance, NaN exactly where the restatement has NaN, and the counts equal."""
    want, n_band = RN.site_values(recs, slon, slat, r_out, stat, **prof)
    assert n_band == 0
    assert not RN.near_threshold(want, thr).any()
    got = res[KEY[stat]]
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    err = np.abs(got - want) - (RN.TOL_ABS + RN.TOL_REL * np.abs(want))
    print('%s: %d values, largest |got - want| = %.3g, largest relative = %.3g'
          % (stat, (~np.isnan(want)).sum(), np.nanmax(np.abs(got - want)), np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))))
    assert RN.close(got, want).all(), [(int(i), int(s), got[i, s], want[i, s]) for i, s in np.argwhere(err > 0)[:5]]
    assert np.array_equal(res['counts'], RN.counts(want, groups, n_groups, thr))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('stat', ['total', 'peak-rate'])
@pytest.mark.parametrize('sub', [1, 3])
def test_gpu_stress_matches_restatement(built_lib, stat, sub):
    from tropical_cyclone_risk_amd import rainfall
    rng = np.random.default_rng(41)
    lon, lat, v = _stress_tracks(rng)
    n_trk = lon.shape[0]
    groups, n_groups = _groups(rng, n_trk)
    r_out = 400.0
    slon, slat = _stress_sites(rng, lon, lat, v, r_out)
    thr = THR_TOTAL if stat == 'total' else THR_PEAK
    recs = RN.records(lon, lat, v, DT, sub)
    assert [None if r is None else r.shape[1] for r in recs[:6]] == [None, None, 1 + sub, 32 * sub + 1, 33 * sub + 1, 11 * sub + 1]
    r = rainfall.site_rain(lon, lat, v, groups, slon, slat, DT, stat=stat, r_out_km=r_out, substeps=sub, thresholds=thr,
                           return_values=True, n_groups=n_groups)
    want = _check(r, stat, recs, groups, n_groups, slon, slat, r_out, thr)
    assert np.isnan(want[:, :2]).all() and np.isnan(want[:, FAR]).all()
    assert want[0, 2] > 0                                                # r = 0: the site at a sample of the 2-sample storm
    assert (r['counts'][:, 1] == 0).all() and (r['counts'][:, 4] == 0).all() and r['counts'].sum() > 200
    assert (~np.isnan(want)).sum() > 300 and not np.isnan(want[1]).all()           # the pole-ward site is rained on


@pytest.mark.gpu
def test_gpu_other_coefficients_and_clamp(built_lib):
    """A coefficient set with T0 < 0 (the rate is clamped at 0 around the centre) and a narrower clamp."""
    from tropical_cyclone_risk_amd import rainfall
    rng = np.random.default_rng(43)
    lon, lat, v = _stress_tracks(rng)
    groups, n_groups = _groups(rng, lon.shape[0])
    slon, slat = _stress_sites(rng, lon, lat, v, 250.0)
    prof = dict(a=(-6.0, -1.0, 70.0, 120.0), b=(3.0, 4.0, -12.0, -10.0), v_lo_kt=40.0, v_hi_kt=140.0)
    recs = RN.records(lon, lat, v, DT, 2)
    r = rainfall.site_rain(lon, lat, v, groups, slon, slat, DT, r_out_km=250.0, substeps=2, thresholds=THR_TOTAL,
                           coefficients=(prof['a'], prof['b']), v_lo_kt=40.0, v_hi_kt=140.0, return_values=True, n_groups=n_groups)
    want = _check(r, 'total', recs, groups, n_groups, slon, slat, 250.0, THR_TOTAL, **prof)
    assert (~np.isnan(want)).sum() > 250 and (want > 0.0).sum() > 250


def _golden():
    lon, lat, vmax = [], [], []
    for b in ('NA', 'AU', 'GL'):
        d = np.load(os.path.join(GOLDEN, 'tracks_%s.npz' % b))
        lon.append(d['traj'][:, 0]); lat.append(d['traj'][:, 1]); vmax.append(d['vmax'])
    return np.concatenate(lon), np.concatenate(lat), np.concatenate(vmax)


@pytest.mark.gpu
@pytest.mark.parametrize('stat', ['total', 'peak-rate'])
def test_gpu_golden_tracks_on_a_site_grid(built_lib, stat):
    from tropical_cyclone_risk_amd import rainfall
    lon, lat, vmax = _golden()
    n_trk = lon.shape[0]
    groups = np.arange(n_trk) % 3
    glon, glat = np.meshgrid(np.arange(-100.3, 361.0, 8.0), np.arange(-48.3, 49.0, 8.0))
    slon, slat = glon.ravel(), glat.ravel()
    thr = THR_TOTAL if stat == 'total' else THR_PEAK
    recs = RN.records(lon, lat, vmax, DT, 1)
    r = rainfall.site_rain(lon, lat, vmax, groups, slon, slat, DT, stat=stat, thresholds=thr, return_values=True)
    want = _check(r, stat, recs, groups, 3, slon, slat, 500.0, thr)
    assert (~np.isnan(want)).sum() > 500 and r['counts'].sum() > 200


@pytest.mark.gpu
def test_gpu_bit_identical_across_runs_site_order_storm_order_and_site_count(built_lib):
    """The guard of the sum's order guarantee: the storm total of a (site, storm) is the same bits whichever lane, tile and chunk
    computed it and whatever was culled around it."""
    import torch
    from tropical_cyclone_risk_amd import rainfall
    rng = np.random.default_rng(5)
    lon, lat, v = _stress_tracks(rng)
    n_trk = lon.shape[0]
    groups, n_groups = _groups(rng, n_trk)
    slon, slat = _stress_sites(rng, lon, lat, v, 500.0)
    dev = torch.device('cuda', 0)
    tl, ta, tv, sl, sa = (torch.as_tensor(x, device=dev) for x in (lon, lat, v, slon, slat))
    for stat, thr in (('total', THR_TOTAL), ('peak-rate', THR_PEAK)):
        kw = dict(stat=stat, r_out_km=500.0, substeps=3, thresholds=thr, return_values=True, n_groups=n_groups)
        key = KEY[stat]

        def same(x, y):
            return torch.equal(x.view(torch.int64), y.view(torch.int64))           # bits: NaN equal to NaN
        a = rainfall.site_rain(tl, ta, tv, groups, sl, sa, DT, **kw)
        assert (~torch.isnan(a[key])).sum() > 500
        b = rainfall.site_rain(tl, ta, tv, groups, sl, sa, DT, **kw)
        assert same(a[key], b[key]) and torch.equal(a['counts'], b['counts'])
        ps = torch.as_tensor(rng.permutation(slon.size), device=dev)
        c = rainfall.site_rain(tl, ta, tv, groups, sl[ps], sa[ps], DT, **kw)
        assert same(c[key], a[key][ps]) and torch.equal(c['counts'], a['counts'][ps])
        pt = np.arange(n_trk)                                               # storms permuted within their groups
        for g in range(n_groups):
            i = np.nonzero(groups == g)[0]
            pt[i] = rng.permutation(i)
        assert np.array_equal(groups[pt], groups) and not np.array_equal(pt, np.arange(n_trk))
        tp = torch.as_tensor(pt, device=dev)
        d = rainfall.site_rain(tl[tp], ta[tp], tv[tp], groups, sl, sa, DT, **kw)
        assert same(d[key], a[key][:, tp]) and torch.equal(d['counts'], a['counts'])
        px = rng.permutation(n_trk)                                         # ... and across groups, the groups going along
        tx = torch.as_tensor(px, device=dev)
        e = rainfall.site_rain(tl[tx], ta[tx], tv[tx], groups[px], sl, sa, DT, **kw)
        assert same(e[key], a[key][:, tx]) and torch.equal(e['counts'], a['counts'])
        # 200 far sites more: other tiles, another grid, the same 70 rows
        fl_ = torch.as_tensor(rng.uniform(0.0, 40.0, 200), device=dev)
        fa_ = torch.as_tensor(rng.uniform(55.0, 80.0, 200), device=dev)
        f = rainfall.site_rain(tl, ta, tv, groups, torch.cat([sl, fl_]), torch.cat([sa, fa_]), DT, **kw)
        assert same(f[key][:70], a[key]) and torch.equal(f['counts'][:70], a['counts'])
        assert torch.isnan(f[key][70:]).all() and int(f['counts'][70:].sum()) == 0


@pytest.mark.gpu
def test_gpu_host_and_device_entry_points_agree_and_pairs(built_lib):
    import torch
    from tropical_cyclone_risk_amd import _lib, rainfall
    from tropical_cyclone_risk_amd.engine import TCEngine
    rng = np.random.default_rng(8)
    lon, lat, v = _stress_tracks(rng)
    n_trk = lon.shape[0]
    groups, n_groups = _groups(rng, n_trk)
    slon, slat = _stress_sites(rng, lon, lat, v, 400.0)
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(x, device=dev) for x in (lon, lat, v, slon, slat)]
    eng = TCEngine('NA', device=0)
    L = _lib.lib()
    pairs = ctypes.c_int64(-1)
    side = torch.cuda.Stream(dev)
    try:
        # no rainfall call on this context yet: an error with a message, not a number
        assert L.tcr_rainfall_pairs(eng.h, ctypes.byref(pairs)) == -1
        assert L.tcr_last_error(eng.h).decode().startswith('tcr_rainfall_pairs: no tcr_rainfall_* call')
        for stat, thr in (('total', THR_TOTAL), ('peak-rate', THR_PEAK)):
            kw = dict(stat=stat, r_out_km=400.0, substeps=4, thresholds=thr, return_values=True, n_groups=n_groups)
            ref = rainfall.site_rain(lon, lat, v, groups, slon, slat, DT, engine=eng, **kw)           # _host
            assert L.tcr_rainfall_pairs(eng.h, ctypes.byref(pairs)) == 0
            n_rec = sum((int(k) - 1) * 4 + 1 for k in RN.track_length(lon, lat, v) if k >= 2)
            assert 0 < pairs.value <= n_rec * slon.size
            for _ in range(2):
                with torch.cuda.stream(side):
                    r = rainfall.site_rain(t[0], t[1], t[2], groups, t[3], t[4], DT, engine=eng, **kw)  # _dev
                side.synchronize()
                assert r['counts'].device == dev and r[KEY[stat]].device == dev
                assert np.array_equal(r['counts'].cpu().numpy(), ref['counts'])
                assert np.array_equal(r[KEY[stat]].cpu().numpy().view(np.int64), ref[KEY[stat]].view(np.int64))
        # no storms at all
        z = rainfall.site_rain(lon[:0], lat[:0], v[:0], groups[:0], slon, slat, DT, return_values=True, n_groups=2, engine=eng)
        assert z['counts'].shape == (70, 2, 10) and z['counts'].sum() == 0 and z['site_total'].shape == (70, 0)
        zt = rainfall.site_rain(t[0][:0], t[1][:0], t[2][:0], groups[:0], t[3], t[4], DT, n_groups=2, engine=eng)
        assert int(zt['counts'].sum()) == 0
        assert L.tcr_rainfall_pairs(eng.h, ctypes.byref(pairs)) == 0 and pairs.value == 0
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
        thr = np.array([10.0, 20.0])
        counts = np.zeros((1, 1, 2), np.int32)
        a0, b0 = (-1.10, -1.60, 64.5, 150.0), (3.96, 4.80, -13.0, -16.0)

        def call(a=a0, b=b0, n_bin=2, n_t_=n_t, **p):
            trk = _lib.HazardTracks(n_trk=n_trk, n_t=n_t_, row_stride=n_t, lon=planes[0].ctypes.data, lat=planes[1].ctypes.data,
                                    vmax=planes[2].ctypes.data, n_group=1, group_off=off)
            prm = _lib.RainParams(**dict(dict(dt_s=DT, r_out_km=500.0, v_lo_kt=35.0, v_hi_kt=155.0, a=(ctypes.c_double * 4)(*a),
                                              b=(ctypes.c_double * 4)(*b), substeps=1, stat=0), **p))
            return L.tcr_rainfall_host(h, ctypes.byref(trk), ctypes.byref(prm), 1, s[0].ctypes.data, s[1].ctypes.data, n_bin,
                                       thr.ctypes.data_as(_lib.DP), counts.ctypes.data, None)
        pairs = ctypes.c_int64()
        rejected = [dict(r_out_km=2001.0), dict(r_out_km=0.0), dict(substeps=0), dict(substeps=65), dict(dt_s=0.0), dict(dt_s=math.inf),
                    dict(stat=2), dict(stat=-1), dict(v_lo_kt=0.0), dict(v_lo_kt=160.0), dict(v_hi_kt=math.inf), dict(v_hi_kt=170.0),
                    dict(a=(math.nan,) + a0[1:]), dict(b=b0[:3] + (math.inf,)), dict(b=(3.96, 4.80, -14.0, -16.0)),
                    dict(b=(3.96, 4.80, -13.0, -40.0)), dict(a=(-1.10, -6.0, 64.5, 150.0)), dict(n_bin=0), dict(n_bin=65),
                    dict(n_t_=0), dict(n_t_=n_t + 1)]
        for p in rejected:
            assert call(**p) == -1, p
            assert L.tcr_last_error(h).decode().startswith('tcr_rainfall:'), (p, L.tcr_last_error(h))
        # none of them got as far as a launch: the context has still seen no rainfall call
        assert L.tcr_rainfall_pairs(h, ctypes.byref(pairs)) == -1
        assert call() == 0 and counts.sum() > 0
        assert L.tcr_rainfall_pairs(h, ctypes.byref(pairs)) == 0 and pairs.value == n_trk * n_t
        assert call(stat=1) == 0
        assert call(a=(-10.0,) + a0[1:]) == 0                              # T0 < 0 is allowed
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_rainfall_next_to_a_footprint_on_two_streams(built_lib):
    """The context's fourth workspace: a rainfall call and a footprint call in flight on two streams of one context give what
    they give one after the other."""
    import torch
    from tropical_cyclone_risk_amd import rainfall, windfield
    from tropical_cyclone_risk_amd.engine import TCEngine
    rng = np.random.default_rng(12)
    lon, lat, v = _stress_tracks(rng)
    n_trk, n_t = lon.shape
    groups, n_groups = _groups(rng, n_trk)
    slon, slat = _stress_sites(rng, lon, lat, v, 500.0)
    env = [rng.normal(0, 8, (n_trk, n_t)) for _ in range(4)]
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(x, device=dev) for x in [lon, lat, v, slon, slat] + env]
    eng = TCEngine('NA', device=0)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)

    def rain():
        return rainfall.site_rain(t[0], t[1], t[2], groups, t[3], t[4], DT, substeps=4, thresholds=THR_TOTAL, return_values=True,
                                  n_groups=n_groups, engine=eng)

    def wind():
        return windfield.site_wind(t[0], t[1], 0.8 * t[2], t[5:9], groups, t[3], t[4], DT, substeps=4, return_max=True,
                                   n_groups=n_groups, engine=eng)
    try:
        r0 = rain()
        w0 = wind()
        torch.cuda.synchronize(dev)
        for _ in range(3):
            with torch.cuda.stream(s1):
                r1 = rain()
            with torch.cuda.stream(s2):
                w1 = wind()
            s1.synchronize()
            s2.synchronize()
            assert torch.equal(r1['site_total'].view(torch.int64), r0['site_total'].view(torch.int64))
            assert torch.equal(w1['site_max'].view(torch.int64), w0['site_max'].view(torch.int64))
            assert torch.equal(r1['counts'], r0['counts']) and torch.equal(w1['counts'], w0['counts'])
        assert int(r0['counts'].sum()) > 0 and int(w0['counts'].sum()) > 0
    finally:
        eng.close()


def _nl(**over):
    from tropical_cyclone_risk_amd import namelist
    nl = types.SimpleNamespace(**{k: getattr(namelist, k) for k in dir(namelist) if not k.startswith('__')})
    for k, val in over.items():
        setattr(nl, k, val)
    return nl


@pytest.mark.gpu
def test_gpu_run_downscaling_tracks_then_cli(golden_env, built_lib, tmp_path):
    from tropical_cyclone_risk_amd import analysis, compute, hazard, io as tio, rainfall
    nl = _nl(start_year=2001, end_year=2003, tracks_per_year=40, dataset_type='SYNTHETIC', output_directory=str(tmp_path), exp_name='rf')
    os.makedirs(tmp_path / 'rf', exist_ok=True)
    fn = compute.run_downscaling('NA', env=golden_env, nl=nl)
    d = tio.read_tracks(fn)
    lon, lat, vmax = (np.asarray(d[k], float) for k in ('lon_trks', 'lat_trks', 'vmax_trks'))
    dt = analysis.sample_spacing([d['time']])
    groups = np.asarray(d['tc_years']).astype(int) - 2001
    i = np.argwhere(np.isfinite(lon) & np.isfinite(vmax))[::53][:8]
    slon = np.concatenate([lon[i[:, 0], i[:, 1]] - 360.0, [-80.1918]])
    slat = np.concatenate([lat[i[:, 0], i[:, 1]] + 0.7, [25.7617]])
    out = str(tmp_path / 'rain.npz')
    cmd = [sys.executable, '-m', 'tropical_cyclone_risk_amd.rainfall', fn, '--out', out, '--substeps', '4', '--thresholds', '5:100:5']
    cmd += ['--site=%.12f,%.12f' % (a, b) for a, b in zip(slon, slat)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert 'return period' in p.stdout and '(mm)' in p.stdout
    z = np.load(out)
    assert set(z.files) == {'counts', 'return_period', 'thresholds', 'site_lon', 'site_lat', 'total_years', 'r_out_km', 'substeps',
                            'stat', 'dt_s', 'group_file', 'group_year', 'files'}
    assert int(z['total_years']) == 3 and z['group_year'].tolist() == [2001, 2002, 2003] and int(z['substeps']) == 4
    assert str(z['stat']) == 'total' and float(z['dt_s']) == dt
    thr = np.arange(5.0, 101.0, 5.0)
    assert np.array_equal(z['thresholds'], thr)
    api = rainfall.site_rain(lon, lat, vmax, groups, z['site_lon'], z['site_lat'], dt, substeps=4, thresholds=thr, n_groups=3,
                             return_values=True)
    assert np.array_equal(z['counts'], api['counts']) and api['counts'].sum() > 0
    rp = z['return_period']
    assert np.array_equal(rp, hazard.return_periods(api['counts'], 3))
    c = z['counts'].sum(axis=1)
    assert np.isfinite(rp[c > 0]).all() and (rp[c > 0] > 0).all() and np.isinf(rp[c == 0]).all()
    # the API's values are the restatement's on this file too
    want, _ = RN.site_values(RN.records(lon, lat, vmax, dt, 4), z['site_lon'], z['site_lat'], 500.0)
    assert RN.close(api['site_total'], want).all()
