"""Site wind hazard (tropical_cyclone_risk_amd/hazard.py, csrc/tcr_hazard.hip): the reference notebook's near-site intensity,
exceedance counts and return periods.  CPU tests check the NumPy restatement against the notebook's own numbers, the host-side
helpers, the CLI plumbing and the C struct layout; GPU tests (`-m gpu`) check the kernels against the restatement."""
import ctypes
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest

from tests import hazard_numpy as HN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def _golden():
    g = np.load(os.path.join(GOLDEN, 'hazard_golden.npz'))
    lon, lat, vmax = [], [], []
    for b in ('NA', 'GL'):
        d = np.load(os.path.join(GOLDEN, 'tracks_%s.npz' % b))
        lon.append(d['traj'][:, 0]); lat.append(d['traj'][:, 1]); vmax.append(d['vmax'])
    return g, np.concatenate(lon), np.concatenate(lat), np.concatenate(vmax)


def _nl(**over):
    from tropical_cyclone_risk_amd import namelist
    nl = types.SimpleNamespace(**{k: getattr(namelist, k) for k in dir(namelist) if not k.startswith('__')})
    for k, v in over.items():
        setattr(nl, k, v)
    return nl


def _random_tracks(rng, n_trk, n_t, lon0=(260, 350), lat0=(5, 45)):
    """Random walks with NaN tails, NaN vmax holes and longitudes above 360."""
    lon = rng.uniform(*lon0, (n_trk, 1)) + np.cumsum(rng.normal(0, 0.4, (n_trk, n_t)), axis=1)
    lat = np.clip(rng.uniform(*lat0, (n_trk, 1)) + np.cumsum(rng.normal(0.05, 0.3, (n_trk, n_t)), axis=1), -89.9, 89.9)
    vmax = rng.uniform(0, 90, (n_trk, n_t))
    end = rng.integers(0, n_t + 1, n_trk)
    tail = np.arange(n_t)[None, :] >= end[:, None]
    lon[tail] = lat[tail] = vmax[tail] = np.nan
    vmax[rng.random((n_trk, n_t)) < 0.02] = np.nan
    return lon, lat, vmax


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_restatement_reproduces_the_notebook_golden():
    g, lon, lat, vmax = _golden()
    R = float(g['radius_km'])
    m, amb = HN.site_max(lon, lat, vmax, g['site_lon'], g['site_lat'], R)
    assert not amb.any()
    assert np.array_equal(m, g['site_max'], equal_nan=True)
    assert (~np.isnan(m)).sum() > 40                      # sites were placed near the tracks
    c = HN.counts(m, g['groups'], 5, g['thresholds'])
    assert np.array_equal(c, g['counts'])
    assert np.array_equal(HN.return_period(c, 5), g['return_period'])
    from tropical_cyclone_risk_amd import hazard
    assert np.array_equal(hazard.return_periods(g['counts'], 5), g['return_period'])


def test_return_periods_and_storm_frequency_by_hand():
    from tropical_cyclone_risk_amd import hazard
    from tropical_cyclone_risk_amd.basins import BASIN_IDS
    c = np.array([[[4, 1, 0], [6, 1, 0]]])                  # one site, two groups, three bins
    rp = hazard.return_periods(c, 20)
    assert rp.shape == (1, 3) and rp[0, 0] == 2.0 and rp[0, 1] == 10.0 and np.isinf(rp[0, 2])
    assert np.array_equal(hazard.return_periods(np.array([[5, 0]]), 10), [[2.0, np.inf]])
    # two ensemble files x three years: seeds summed over files and months, gamma = tpy / seeds, f = obs / mean(gamma) * gamma
    spm = np.zeros((2, 3, len(BASIN_IDS), 12))
    na = BASIN_IDS.index('NA')
    spm[:, 0, na, 5] = 10; spm[:, 1, na, 6] = 20; spm[:, 2, na, 7] = 40
    spm[:, :, BASIN_IDS.index('EP'), :] = 99                # other basins do not enter
    f = hazard.storm_frequency(spm, 'NA', 14, 7)
    gamma = 14 / np.array([20.0, 40.0, 80.0])
    assert np.allclose(f, 7 / gamma.mean() * gamma, rtol=0, atol=1e-12) and np.isclose(f.mean(), 7)
    assert np.allclose(hazard.storm_frequency(spm[0], 'NA', 14, 7), f)      # one file: [year][basin][month]


def test_thresholds_and_grid_parsing():
    from tropical_cyclone_risk_amd import hazard
    a = hazard.parse_args(['x.nc', '--site=-80.19,25.76', '--site', '280,30', '--grid', '270:271:0.5,20:21:1',
                           '--thresholds', '10:80:5', '--radius-km', '150'])
    assert np.array_equal(a.thresholds, np.arange(10, 81, 5)) and a.radius_km == 150.0
    lon, lat = hazard.collect_sites(a)
    assert lon.tolist() == [-80.19, 280, 270, 270.5, 271, 270, 270.5, 271]
    assert lat.tolist() == [25.76, 30, 20, 20, 20, 21, 21, 21]
    b = hazard.parse_args(['x.nc', '--site', '1,2'])
    assert np.array_equal(b.thresholds, hazard.DEFAULT_THRESHOLDS) and b.out == 'hazard.npz'
    with pytest.raises(SystemExit):
        hazard.parse_args(['x.nc'])                               # no sites
    with pytest.raises(SystemExit):
        hazard.parse_args(['x.nc', '--site', '1,2', '--thresholds', '10:5:1'])
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, 's.csv')
        open(fn, 'w').write('lon,lat\n-80.2,25.8\n\n10;20\n')
        assert hazard.read_sites_csv(fn) == [(-80.2, 25.8), (10.0, 20.0)]


def _write_two_files(tmp_path, rng):
    from tropical_cyclone_risk_amd import io as tio
    from tropical_cyclone_risk_amd.basins import TC_Basin
    nl = _nl(output_directory=str(tmp_path), exp_name='hz', start_year=2001, end_year=2003)
    ns = 361

    def year(n):
        lon, lat, vmax = _random_tracks(rng, n, ns)
        return (lon, lat, vmax, vmax, vmax, rng.random((n, ns, 4)), rng.integers(1, 13, n).astype(float),
                np.array(['NA'] * n, dtype='U2'), rng.integers(0, 9, (7, 12)).astype(float))
    f0 = tio.write_tracks([year(3), year(0), year(4)], [2001, 2002, 2003], TC_Basin('NA'), nl)
    f1 = tio.write_tracks([year(2), year(5), year(1)], [2001, 2002, 2003], TC_Basin('NA'), nl)
    return f0, f1


def test_cli_group_map_over_two_files(tmp_path):
    from tropical_cyclone_risk_amd import hazard, io as tio
    f0, f1 = _write_two_files(tmp_path, np.random.default_rng(3))
    assert f1.endswith('_e0.nc')
    lon, lat, vmax, groups, gfile, gyear = hazard.load_groups([f0, f1])
    assert lon.shape == (15, 361)
    assert gfile.tolist() == [0, 0, 0, 1, 1, 1] and gyear.tolist() == [2001, 2002, 2003] * 2
    assert groups.tolist() == [0] * 3 + [2] * 4 + [3] * 2 + [4] * 5 + [5]              # file 0 has no storm in 2002
    d0 = tio.read_tracks(f0)
    assert np.array_equal(lon[:7], d0['lon_trks'], equal_nan=True)
    assert np.array_equal(vmax[7:], tio.read_tracks(f1)['vmax_trks'], equal_nan=True)


def test_grouping_unsorted_and_empty_groups_in_the_restatement():
    smax = np.array([[30.0, np.nan, 50.0, 12.0]])
    c = HN.counts(smax, [2, 0, 2, 0], 4, [10.0, 40.0])
    assert c.tolist() == [[[1, 0], [0, 0], [2, 1], [0, 0]]]


def test_hazard_struct_layout_matches_header():
    from tropical_cyclone_risk_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tcrisk_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
           'sizeof(tcr_hazard_tracks),offsetof(tcr_hazard_tracks, lon),offsetof(tcr_hazard_tracks, vmax),'
           'offsetof(tcr_hazard_tracks, n_group),offsetof(tcr_hazard_tracks, group_off));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'sz.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 'sz')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    H = _lib.HazardTracks
    assert sizes == [ctypes.sizeof(H), H.lon.offset, H.vmax.offset, H.n_group.offset, H.group_off.offset]


def test_hazard_symbols_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_hazard_dev', 'tcr_hazard_host', 'tcr_hazard_pairs'):
        assert hasattr(L, name), name


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_golden_bit_identical(built_lib):
    from tropical_cyclone_risk_amd import hazard
    g, lon, lat, vmax = _golden()
    r = hazard.site_hazard(lon, lat, vmax, g['groups'], g['site_lon'], g['site_lat'], radius_km=float(g['radius_km']),
                           thresholds=g['thresholds'], return_max=True, n_groups=5)
    assert np.array_equal(r['site_max'].view(np.int64), g['site_max'].view(np.int64))       # bit-identical, NaN included
    assert r['counts'].dtype == np.int32 and np.array_equal(r['counts'], g['counts'])
    assert np.array_equal(hazard.return_periods(r['counts'], int(g['total_years'])), g['return_period'])


def _stress_case(rng):
    n_t = 100
    parts = [_random_tracks(rng, 260, n_t), _random_tracks(rng, 30, n_t, lon0=(170, 190), lat0=(-30, 30)),
             _random_tracks(rng, 20, n_t, lon0=(0, 360), lat0=(80, 88))]
    lon, lat, vmax = (np.concatenate([p[k] for p in parts]) for k in range(3))
    n_trk = lon.shape[0]
    # groups: one group larger than a chunk (most storms), empty groups 1 and 4, a one-storm group 3, unsorted
    groups = np.full(n_trk, 0)
    groups[rng.choice(n_trk, 40, replace=False)] = 2
    groups[7] = 3
    rng.shuffle(groups)
    live = np.argwhere(~np.isnan(lon))
    pick = live[rng.choice(len(live), 150, replace=False)]
    R = 100.0
    # sites exactly R from a sample (by the restatement's own distance, up to its rounding), and 0.3 - 1.5 R from samples
    el, ea = HN.offset_point(lon[pick[:80, 0], pick[:80, 1]], lat[pick[:80, 0], pick[:80, 1]], np.full(80, R), rng.uniform(0, 6.3, 80))
    nl_, na_ = HN.offset_point(lon[pick[80:, 0], pick[80:, 1]], lat[pick[80:, 0], pick[80:, 1]], rng.uniform(30, 150, 70),
                            rng.uniform(0, 6.3, 70))
    slon = np.concatenate([el, nl_, nl_ - 360.0, [180.0, -180.0, 179.95, 0.0, 45.0, 200.0], rng.uniform(-180, 360, 40)])
    slat = np.concatenate([ea, na_, na_, [10.0, 10.0, -5.0, 89.95, -89.9, 86.0], rng.uniform(-60, 60, 40)])
    return lon, lat, vmax, groups, slon, slat, R


@pytest.mark.gpu
def test_gpu_stress_matches_restatement(built_lib):
    from tropical_cyclone_risk_amd import hazard
    rng = np.random.default_rng(11)
    lon, lat, vmax, groups, slon, slat, R = _stress_case(rng)
    for thr in (np.array([35.0]), np.linspace(0.0, 90.0, 64)):
        r = hazard.site_hazard(lon, lat, vmax, groups, slon, slat, radius_km=R, thresholds=thr, return_max=True, n_groups=5)
        ok = HN.allowed(r['site_max'], lon, lat, vmax, slon, slat, R)
        assert ok.all(), np.argwhere(~ok)[:5]
        assert np.array_equal(r['counts'], HN.counts(r['site_max'], groups, 5, thr))
        assert (r['counts'][:, 1] == 0).all() and (r['counts'][:, 4] == 0).all()
    m_lo, amb = HN.site_max(lon, lat, vmax, slon, slat, R)
    assert (~np.isnan(r['site_max'])).sum() > 300
    print('stress: %d ambiguous pairs, %d (site, storm) maxima' % (int(amb.sum()), int((~np.isnan(m_lo)).sum())))


@pytest.mark.gpu
def test_gpu_device_tensors_on_a_side_stream(built_lib):
    import torch
    from tropical_cyclone_risk_amd import hazard
    from tropical_cyclone_risk_amd.engine import TCEngine
    rng = np.random.default_rng(5)
    lon, lat, vmax, groups, slon, slat, R = _stress_case(rng)
    thr = np.arange(10, 81, 5).astype(float)
    ref = hazard.site_hazard(lon, lat, vmax, groups, slon, slat, radius_km=R, thresholds=thr, return_max=True, n_groups=5)
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(a, device=dev) for a in (lon, lat, vmax, slon, slat)]
    eng = TCEngine('NA', device=0)
    side = torch.cuda.Stream(dev)
    runs = []
    for _ in range(2):
        with torch.cuda.stream(side):
            r = hazard.site_hazard(t[0], t[1], t[2], groups, t[3], t[4], radius_km=R, thresholds=thr, return_max=True,
                                   engine=eng, n_groups=5)
        side.synchronize()
        assert r['counts'].device == dev and r['site_max'].device == dev
        runs.append((r['counts'].cpu().numpy(), r['site_max'].cpu().numpy()))
    eng.close()
    for c, m in runs:
        assert np.array_equal(c, ref['counts'])
        assert np.array_equal(m.view(np.int64), ref['site_max'].view(np.int64))


@pytest.mark.gpu
def test_gpu_bad_arguments_raise(built_lib):
    from tropical_cyclone_risk_amd import hazard, _lib
    rng = np.random.default_rng(1)
    lon, lat, vmax = _random_tracks(rng, 8, 20)
    g = np.zeros(8, dtype=np.int64)
    s = (np.array([280.0]), np.array([20.0]))
    for kw in (dict(radius_km=0.0), dict(radius_km=5001.0), dict(radius_km=np.nan), dict(thresholds=np.array([20.0, 10.0])),
               dict(thresholds=np.array([10.0, np.inf])), dict(thresholds=np.arange(65.0)), dict(thresholds=np.array([]))):
        with pytest.raises(_lib.TcrError):
            hazard.site_hazard(lon, lat, vmax, g, *s, **kw)
    # the ABI checks group_off itself
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        off = (ctypes.c_int64 * 3)(0, 5, 4)
        trk = _lib.HazardTracks(n_trk=4, n_t=20, row_stride=20, lon=lon.ctypes.data, lat=lat.ctypes.data, vmax=vmax.ctypes.data,
                                n_group=2, group_off=off)
        counts = np.zeros((1, 2, 1), np.int32)
        thr = np.array([10.0])
        rc = L.tcr_hazard_host(h, ctypes.byref(trk), 1, s[0].ctypes.data, s[1].ctypes.data, 100.0, 1,
                               thr.ctypes.data_as(_lib.DP), counts.ctypes.data, None)
        assert rc == -1 and b'group_off' in L.tcr_last_error(h)
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_end_to_end_run_downscaling_then_cli(golden_env, built_lib, tmp_path):
    from tropical_cyclone_risk_amd import compute, io as tio
    nl = _nl(start_year=2001, end_year=2003, tracks_per_year=50, dataset_type='SYNTHETIC', output_directory=str(tmp_path),
             exp_name='hz')
    os.makedirs(tmp_path / 'hz', exist_ok=True)
    fn = compute.run_downscaling('NA', env=golden_env, nl=nl)
    d = tio.read_tracks(fn)
    lon, lat, vmax = (np.asarray(d[k], float) for k in ('lon_trks', 'lat_trks', 'vmax_trks'))
    i = np.argwhere(~np.isnan(lon))[::97][:6]
    sites = ['%.10f,%.10f' % (lon[a, b] - 360.0, lat[a, b] + 0.5) for a, b in i] + ['-80.1918,25.7617']
    out = str(tmp_path / 'hazard.npz')
    cmd = [sys.executable, '-m', 'tropical_cyclone_risk_amd.hazard', fn, '--out', out, '--thresholds', '10:80:5']
    for s in sites:
        cmd += ['--site=' + s]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert 'return period' in p.stdout
    z = np.load(out)
    assert set(z.files) == {'counts', 'return_period', 'thresholds', 'site_lon', 'site_lat', 'total_years', 'radius_km', 'group_file',
                            'group_year', 'files'}
    assert int(z['total_years']) == 3 and z['group_year'].tolist() == [2001, 2002, 2003] and z['group_file'].tolist() == [0, 0, 0]
    groups = np.asarray(d['tc_years']).astype(int) - 2001
    m_lo, amb = HN.site_max(lon, lat, vmax, z['site_lon'], z['site_lat'], 100.0)
    assert not amb.any()
    want = HN.counts(m_lo, groups, 3, np.arange(10, 81, 5))
    assert np.array_equal(z['counts'], want) and want.sum() > 0
    assert np.array_equal(z['return_period'], HN.return_period(want, 3))
