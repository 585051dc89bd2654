"""Track climatology (tropical_cyclone_risk_amd/climatology.py, csrc/tcr_climatology.hip): track, exceedance, genesis and LMI
counts and PDI per cell and group, per-storm genesis / LMI / PDI, the host aggregates and the CLI.  CPU tests pin the NumPy
restatement (tests/climatology_numpy.py) to hand-computed results and check the aggregates, the CLI plumbing and the C struct
layouts; GPU tests (`-m gpu`) check the kernel against the restatement with `==` (floats as int64 bit patterns)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import climatology_numpy as CN
from tropical_cyclone_risk_amd import climatology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nan = np.nan
G1 = (0.0, 30.0, 12, -60.0, 30.0, 4)                     # global: 12 x 4 cells of 30 degrees, lat -60..60
R1 = (-100.0, 10.0, 3, 10.0, 10.0, 2)                    # regional: lon 260..290, lat 10..30
V_HALF_ODD, V_HALF_EVEN = 0.4717401446429734, 0.48176492363499956     # ((v * v) * v) * 1024 == 107.5 and 114.5 exactly
THR = (25.0, 40.0)


def _planes(storms):
    n_t = max(len(p) for p in storms)
    a = np.full((3, len(storms), n_t), nan)
    for s, p in enumerate(storms):
        for k, row in enumerate(p):
            a[:, s, k] = row
    return a[0], a[1], a[2]


def _hand_storms():
    A = [(10, 5, 20), (29.9, 5, 30), (nan, nan, 99), (30, 0, 40), (45, 10, nan), (25, 10, 40), (330, 29.999, 10)]
    B = [(x + (-360 if k % 2 == 0 else 360), y, v) for k, (x, y, v) in enumerate(A)]        # both conventions, lon > 360
    C = [(np.nextafter(0.0, -1.0), -60, 5), (np.nextafter(360.0, 0.0), -60, 50), (360.0, 60.0, 60),
         (-30.0, 59.9, 45), (0.0, np.nextafter(-60.0, -90.0), 400.0)]
    D = [(nan, 10, 50), (nan, 10, 60), (20, nan, 70)]                                       # no live sample
    E = [(100, -70, 10), (100, -50, 20), (100, -45, nan)]                                   # genesis outside the grid
    F = [(200, 40, V_HALF_ODD), (200, 40, V_HALF_EVEN), (200, 40, 0.0)]                      # q at half-integers
    return _planes([A, B, C, D, E, F]), np.array([0, 1, 0, 1, 0, 2])


def _q(v):
    return int(np.rint(v ** 3 * 1024))


def _hand_expected():
    """G1, thresholds (25, 40), groups [0, 1, 0, 1, 0, 2]."""
    track = np.zeros((3, 48), np.int32)
    exceed = np.zeros((3, 2, 48), np.int32)
    genesis, lmi = np.zeros_like(track), np.zeros_like(track)
    pdi = np.zeros((3, 48), np.int64)
    for g in (0, 1):                                     # A in group 0, B (= A) in group 1: cells 24 (k 0, 1, 5), 25 (k 3, 4), 35
        track[g, [24, 25, 35]] += 1
        exceed[g, :, 24] += 1; exceed[g, :, 25] += 1     # maxima 40 and 40 (NaN skipped); 10 in cell 35
        genesis[g, 24] += 1
        lmi[g, 25] += 1                                  # the tie 40 at k 3 and 5: the first
        pdi[g, 24] += _q(20) + _q(30) + _q(40); pdi[g, 25] += _q(40); pdi[g, 35] += _q(10)
    # C: cell 0 (lon0 - 1 ulp reduces to 360, then 0), 11 (360 - 1 ulp), 47 (top row), two samples outside (lat 60, -60 - 1 ulp)
    track[0, [0, 11, 47]] += 1
    exceed[0, :, 11] += 1; exceed[0, :, 47] += 1
    genesis[0, 0] += 1
    pdi[0, 0] += _q(5); pdi[0, 11] += _q(50); pdi[0, 47] += _q(45)
    # E: the first sample outside; cell 3 (i 3, j 0)
    track[0, 3] += 1; lmi[0, 3] += 1; pdi[0, 3] += _q(20)
    # F: cell 42; q = rint(107.5) + rint(114.5) + 0 = 108 + 114
    track[2, 42] += 1; genesis[2, 42] += 1; lmi[2, 42] += 1; pdi[2, 42] += 108 + 114
    pa = _q(20) + _q(30) + _q(40) + _q(40) + _q(10)
    shape = (3, 4, 12)
    return dict(track=track.reshape(shape), exceed=exceed.reshape(3, 2, 4, 12), genesis=genesis.reshape(shape), lmi=lmi.reshape(shape),
                pdi=pdi.reshape(shape), genesis_k=np.array([0, 0, 0, -1, 0, 0], np.int32), lmi_k=np.array([3, 3, 4, -1, 1, 1], np.int32),
                lmi_v=np.array([40.0, 40.0, 400.0, nan, 20.0, V_HALF_EVEN]),
                pdi_storm=np.array([pa, pa, _q(5) + _q(50) + _q(60) + _q(45) + _q(400), 0, _q(10) + _q(20), 222], np.int64))


def _assert_equal(got, want):
    for k in climatology.MAP_FIELDS + climatology.STORM_FIELDS:
        a = got[k]
        a = np.asarray(a.cpu() if hasattr(a, 'cpu') else a)
        b = np.asarray(want[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert a.dtype == (np.float64 if k == 'lmi_v' else np.int64 if k in ('pdi', 'pdi_storm') else np.int32), (k, a.dtype)
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)
        assert np.array_equal(a, b), (k, np.argwhere(a != b)[:5])


def _walks(rng, n_trk, n_t, step=0.6, box=(250.0, 20.0)):
    """Slow random walks (they leave cells and come back), NaN gaps and tails, both conventions, lon > 360, vmax in [0, 90]
    with NaN holes."""
    lon = box[0] + rng.uniform(0, 30, (n_trk, 1)) + np.cumsum(rng.normal(0, step, (n_trk, n_t)), axis=1)
    lat = box[1] + rng.uniform(0, 20, (n_trk, 1)) + np.cumsum(rng.normal(0, step, (n_trk, n_t)), axis=1)
    conv = rng.random(n_trk)
    lon[conv < 0.3] -= 360.0
    lon[conv > 0.85] += 360.0
    vmax = np.clip(30 + np.cumsum(rng.normal(0, 2.0, (n_trk, n_t)), axis=1), 0, 90)
    vmax[rng.random(vmax.shape) < 0.05] = nan
    lon[rng.random(lon.shape) < 0.03] = nan
    lat[rng.random(lat.shape) < 0.01] = nan
    end = rng.integers(1, n_t + 1, n_trk)
    tail = np.arange(n_t)[None, :] >= end[:, None]
    lon[tail] = lat[tail] = vmax[tail] = nan
    return lon, lat, vmax


def _stress(rng, n_trk=600, d=1.0):
    """bench_hazard.make_tracks-style tracks; a fifth of the samples snapped to cell edges (lon, lat or both)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import bench_hazard as BH
    lon, lat, vmax, _ = BH.make_tracks(rng, 1, n_trk)
    snap = rng.random(lon.shape)
    lon = np.where(snap < 0.1, np.round(lon / d) * d, lon)
    lat = np.where((snap < 0.05) | ((snap > 0.1) & (snap < 0.2)), np.round(lat / d) * d, lat)
    conv = rng.random(n_trk)
    lon[conv < 0.35] -= 360.0
    lon[conv > 0.9] += 360.0
    return lon, lat, vmax


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_restatement_equals_hand_results():
    (lon, lat, vmax), groups = _hand_storms()
    got = CN.climatology(lon, lat, vmax, groups, 3, G1, THR)
    _assert_equal(got, _hand_expected())


def test_restatement_cell_arithmetic_by_hand():
    x = np.array([265.0, -95.0, 275.0, 295.0, 255.0, 265.0, 625.0, -455.0, 290.0, 260.0, nan])
    y = np.array([15.0, 25.0, 15.0, 15.0, 15.0, 10.0, 29.999, 30.0, 20.0, 9.999, 15.0])
    # regional grid: outside west (255), east (295, and exactly 290), above (30) and below (9.999); lon > 360 and < -360
    assert CN.cells_of(x, y, *R1).tolist() == [0, 3, 1, -1, -1, 0, 3, -1, -1, -1, -1]
    # a global grid whose last column takes 360 - 1 ulp (t / dlon rounds to nlon there); the same spacing regional: outside
    d = 360.0 / 19
    assert 19 * d == 360.0 and np.floor(np.nextafter(360.0, 0.0) / d) == 19
    xs = np.array([np.nextafter(360.0, 0.0), np.nextafter(0.0, -1.0), -1e-14, 0.0, 180.0])
    assert CN.cells_of(xs, np.zeros(5), 0.0, d, 19, -90.0, 180.0, 1).tolist() == [18, 0, 0, 0, 9]
    assert CN.cells_of(xs, np.zeros(5), 0.0, d, 18, -90.0, 180.0, 1).tolist() == [-1, 0, 0, 0, 9]
    # the arithmetic, not the real-number cell: (60 - 1 ulp + 60) / 30 rounds to 4, so 60 - 1 ulp is above the top row
    assert CN.cells_of([-30.0, -30.0], [np.nextafter(60.0, 0.0), 59.9], *G1).tolist() == [-1, 47]
    # q: round half to even at exact half-integers
    assert ((V_HALF_ODD * V_HALF_ODD) * V_HALF_ODD) * 1024.0 == 107.5
    assert ((V_HALF_EVEN * V_HALF_EVEN) * V_HALF_EVEN) * 1024.0 == 114.5
    assert CN.q_of([V_HALF_ODD, V_HALF_EVEN, 400.0, 400.0001, -0.0, -1.0, nan]).tolist() == [108, 114, 65536000000, 0, 0, 0, 0]


def test_regional_grid_by_hand():
    lon = np.array([[265.0, -95.0, 275.0, 295.0, 255.0, 265.0]])
    lat = np.array([[15.0, 25.0, 15.0, 15.0, 15.0, 15.0]])
    vmax = np.array([[30.0, 35.0, 20.0, 70.0, 80.0, 10.0]])
    r = CN.climatology(lon, lat, vmax, [0], 1, R1, THR)
    assert r['track'][0].tolist() == [[1, 1, 0], [1, 0, 0]]
    assert r['exceed'][0, 0].tolist() == [[1, 0, 0], [1, 0, 0]] and r['exceed'][0, 1].sum() == 0
    assert r['genesis'][0].tolist() == [[1, 0, 0], [0, 0, 0]] and r['lmi'].sum() == 0          # LMI at 255 E: outside
    assert r['pdi'][0, 0, 0] == _q(30) + _q(10) and r['pdi_storm'][0] == sum(_q(v) for v in vmax[0])
    assert r['lmi_k'].tolist() == [4]


def test_grid_validation_and_from_bounds():
    g = climatology.CellGrid.from_bounds(0, 360, -90, 90, 1)
    assert (g.nlon, g.nlat, g.is_global) == (360, 180, True)
    g = climatology.CellGrid.from_bounds(260, 350, 0, 60, 0.25)
    assert (g.nlon, g.nlat, g.is_global, g.lon0, g.lat0) == (360, 240, False, 260.0, 0.0)
    assert g.lon_edges[-1] == 350.0 and g.lat_edges.size == 241
    g = climatology.CellGrid.from_bounds(-100, -70, 10, 30, (10, 5))
    assert (g.nlon, g.nlat, g.dlat) == (3, 4, 5.0)
    for bad in ((0, 360, -90, 90, 0.7), (0, 0, 0, 10, 1), (10, 0, 0, 10, 1), (0, 10, 0, 10, 0), (0, 720, 0, 10, 1)):
        with pytest.raises(ValueError):
            climatology.CellGrid.from_bounds(*bad)
    for bad in ((0, 1, 361, 0, 1, 1), (0, -1, 10, 0, 1, 1), (nan, 1, 10, 0, 1, 1), (0, 1, 10, 0, 1, 0), (0, 1e-3, 65536, 0, 1, 32768)):
        with pytest.raises(ValueError):
            climatology.CellGrid(*bad)


def test_host_aggregates_by_hand():
    groups = np.array([0, 2, 0, 1, 2, 2])
    assert climatology.storm_counts(groups, 4).tolist() == [2, 1, 3, 0]
    pdi = np.array([1024, 2048, 3072, 0, 1 << 40, 1], np.int64)
    assert climatology.annual_pdi(pdi, groups, 3600.0, 4).tolist() == [4 * 3600.0, 0.0, (2048 + (1 << 40) + 1) / 1024 * 3600.0, 0.0]
    month = np.array([9.0, 8.0, 9.0, nan, 12.0, 0.0])
    basins = np.array([b'NA', b'EP', b'NA', b'NA', b'NA', b'NA'])
    sc = climatology.seasonal_cycle(month, basins, groups, 3)
    assert sc.shape == (3, 12) and sc[0, 8] == 2 and sc[2, 7] == 1 and sc[2, 11] == 1 and sc.sum() == 4
    sc = climatology.seasonal_cycle(month, np.array(['NA', 'EP', 'NA', 'NA', 'NA ', 'NA']), groups, 3, basin='NA')
    assert sc[0, 8] == 2 and sc[2, 7] == 0 and sc[2, 11] == 1 and sc.sum() == 3
    v = np.array([33.0, 70.0, nan, 10.0, 90.0, 95.0])
    h = climatology.lmi_histogram(v, groups, [0, 33, 50, 90], 3)
    assert h.tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 2]]         # 90 in the closed last bin, 95 outside, NaN not counted
    for g in range(3):
        sel = (groups == g) & ~np.isnan(v)
        assert h[g].tolist() == np.histogram(v[sel], [0, 33, 50, 90])[0].tolist()
    with pytest.raises(ValueError):
        climatology.storm_counts(np.array([0, 5]), 3)
    with pytest.raises(ValueError):
        climatology.lmi_histogram(v, groups, [10, 10], 3)


def test_sample_spacing():
    t = np.linspace(0, 15 * 86400, 361)
    assert climatology.sample_spacing([t, t]) == t[1] - t[0]
    assert climatology.sample_spacing([np.zeros(1)]) == 3600.0
    with pytest.raises(ValueError):
        climatology.sample_spacing([np.array([0.0, 1.0, 3.0])])
    with pytest.raises(ValueError):
        climatology.sample_spacing([t, t * 2])


def test_cli_parsing():
    a = climatology.parse_args(['x.nc', 'y.nc', '--cells', '260:350:0.25,0:60:0.5', '--thresholds', '33,50', '--basin', 'NA',
                                '--per-group', '--out', 'c.npz'])
    assert a.tracks == ['x.nc', 'y.nc'] and a.per_group and a.basin == 'NA' and a.out == 'c.npz'
    assert (a.cells.lon0, a.cells.nlon, a.cells.dlon, a.cells.nlat, a.cells.dlat) == (260.0, 360, 0.25, 120, 0.5)
    assert a.thresholds.tolist() == [33.0, 50.0]
    b = climatology.parse_args(['x.nc'])
    assert (b.cells.nlon, b.cells.nlat, b.cells.is_global, b.per_group, b.basin) == (360, 180, True, False, None)
    assert b.thresholds.tolist() == list(climatology.SAFFIR_SIMPSON) and b.out == 'climatology.npz'
    assert climatology.parse_args(['x.nc', '--thresholds', '20:40:10']).thresholds.tolist() == [20.0, 30.0, 40.0]
    assert climatology.parse_args(['x.nc', '--thresholds', 'none']).thresholds.size == 0
    for bad in (['x.nc', '--cells', '0:360:1'], ['x.nc', '--cells', '0:360:0.7,-90:90:1'], ['x.nc', '--cells', '0:360:1,-90:90'],
                ['x.nc', '--cells', '10:0:1,0:10:1'], ['x.nc', '--cells', '0:720:1,0:10:1'], ['x.nc', '--cells', 'a:b:c,0:1:1'],
                ['x.nc', '--thresholds', '50,40'], ['x.nc', '--thresholds', 'x'], []):
        with pytest.raises(SystemExit):
            climatology.parse_args(bad)


def test_clim_struct_layouts_match_header():
    from tropical_cyclone_risk_amd import _lib
    fields = ('track', 'exceed', 'genesis', 'lmi', 'pdi', 'genesis_k', 'lmi_v', 'lmi_k', 'pdi_storm')
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tcrisk_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n",'
           'sizeof(tcr_clim_grid),offsetof(tcr_clim_grid, dlon),offsetof(tcr_clim_grid, lat0),offsetof(tcr_clim_grid, dlat),'
           'offsetof(tcr_clim_grid, nlon),offsetof(tcr_clim_grid, nlat),sizeof(tcr_clim_out));'
           + ''.join('printf("%%zu\\n", offsetof(tcr_clim_out, %s));' % f for f in fields) + 'return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'sz.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 'sz')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    G, O = _lib.ClimGrid, _lib.ClimOut
    assert sizes[:7] == [ctypes.sizeof(G), G.dlon.offset, G.lat0.offset, G.dlat.offset, G.nlon.offset, G.nlat.offset, ctypes.sizeof(O)]
    assert sizes[7:] == [getattr(O, f).offset for f in fields]


def test_climatology_symbols_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_climatology_dev', 'tcr_climatology_host'):
        assert hasattr(L, name), name


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_hand_built_and_regional(built_lib):
    (lon, lat, vmax), groups = _hand_storms()
    g1 = climatology.CellGrid(*G1)
    _assert_equal(climatology.track_climatology(lon, lat, vmax, groups, g1, THR, n_groups=3), _hand_expected())
    want = CN.climatology(lon, lat, vmax, groups, 3, G1, ())
    _assert_equal(climatology.track_climatology(lon, lat, vmax, groups, g1, n_groups=3), want)       # no thresholds
    rng = np.random.default_rng(5)
    wl, wa, wv = _walks(rng, 300, 200, step=0.8)
    wg = rng.integers(0, 4, 300)
    for grid in (R1, (0.0, 360.0 / 19, 19, -90.0, 180.0 / 7, 7), (0.0, 360.0 / 19, 18, -90.0, 180.0 / 7, 7)):
        want = CN.climatology(wl, wa, wv, wg, 4, grid, (10.0, 30.0, 50.0))
        _assert_equal(climatology.track_climatology(wl, wa, wv, wg, climatology.CellGrid(*grid), (10.0, 30.0, 50.0), n_groups=4), want)
    assert want['track'].sum() > 300


@pytest.mark.gpu
def test_gpu_stress_matches_restatement(built_lib):
    rng = np.random.default_rng(11)
    lon, lat, vmax = _stress(rng, 600, 1.0)
    groups = rng.integers(0, 5, lon.shape[0])
    thr = (20.0, 33.0, 50.0)
    for grid in ((0.0, 1.0, 360, -90.0, 1.0, 180), (260.0, 0.25, 360, 0.0, 0.25, 240)):
        want = CN.climatology(lon, lat, vmax, groups, 5, grid, thr)
        got = climatology.track_climatology(lon, lat, vmax, groups, climatology.CellGrid(*grid), thr, n_groups=5)
        _assert_equal(got, want)
        assert want['track'].sum() > 10000 and want['exceed'][:, 2].sum() > 100
        # a storm that revisits a cell is counted once there: track <= live samples per storm and cell
        assert want['genesis'].sum() + want['lmi'].sum() > 500


@pytest.mark.gpu
@pytest.mark.parametrize('n_t', [1, 63, 64, 65, 361, 700, 1500])
def test_gpu_track_lengths_and_workspace(built_lib, n_t):
    rng = np.random.default_rng(100 + n_t)
    lon, lat, vmax = _walks(rng, 150, n_t, step=0.3)
    groups = rng.integers(0, 3, 150)
    grid = (240.0, 2.0, 40, 0.0, 2.0, 25)
    want = CN.climatology(lon, lat, vmax, groups, 3, grid, THR)
    _assert_equal(climatology.track_climatology(lon, lat, vmax, groups, climatology.CellGrid(*grid), THR, n_groups=3), want)


@pytest.mark.gpu
def test_gpu_host_equals_device_and_engine_side_stream(built_lib):
    import torch
    from tropical_cyclone_risk_amd.engine import TCEngine
    rng = np.random.default_rng(3)
    lon, lat, vmax = _stress(rng, 400, 0.5)
    groups = rng.integers(0, 3, 400)
    grid = climatology.CellGrid.from_bounds(0, 360, -90, 90, 0.5)
    host = climatology.track_climatology(lon, lat, vmax, groups, grid, THR)
    _assert_equal(host, CN.climatology(lon, lat, vmax, groups, 3, (0.0, 0.5, 720, -90.0, 0.5, 360), THR))
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(a, device=dev) for a in (lon, lat, vmax)]
    _assert_equal(climatology.track_climatology(*t, torch.as_tensor(groups, device=dev), grid, THR), host)
    eng = TCEngine('NA', device=0)
    side = torch.cuda.Stream(dev)
    try:
        for _ in range(2):
            with torch.cuda.stream(side):
                r = climatology.track_climatology(*t, groups, grid, THR, engine=eng)
            side.synchronize()
            assert all(r[k].device == dev for k in climatology.MAP_FIELDS + climatology.STORM_FIELDS)
            _assert_equal(r, host)
        # tracks beyond the LDS slice: the context's workspace, grown and then reused
        ll, la, lv = _walks(rng, 50, 900, step=0.3)
        lg = rng.integers(0, 2, 50)
        g2 = climatology.CellGrid(240.0, 2.0, 40, 0.0, 2.0, 25)
        want = CN.climatology(ll, la, lv, lg, 2, (240.0, 2.0, 40, 0.0, 2.0, 25), THR)
        for _ in range(2):
            with torch.cuda.stream(side):
                r = climatology.track_climatology(*[torch.as_tensor(a, device=dev) for a in (ll, la, lv)], lg, g2, THR, engine=eng)
            side.synchronize()
            _assert_equal(r, want)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_storm_order_does_not_matter(built_lib):
    rng = np.random.default_rng(17)
    lon, lat, vmax = _stress(rng, 500, 1.0)
    groups = rng.integers(0, 4, 500)
    grid = climatology.CellGrid.from_bounds(200, 360, 0, 60, 1)
    a = climatology.track_climatology(lon, lat, vmax, groups, grid, THR, n_groups=4)
    p = rng.permutation(500)
    b = climatology.track_climatology(lon[p], lat[p], vmax[p], groups[p], grid, THR, n_groups=4)
    for k in climatology.MAP_FIELDS:
        assert np.array_equal(a[k], b[k]), k
    for k in climatology.STORM_FIELDS:
        x, y = a[k][p], b[k]
        if k == 'lmi_v':
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), k


@pytest.mark.gpu
def test_gpu_bad_arguments_and_empty(built_lib):
    from tropical_cyclone_risk_amd import _lib
    (lon, lat, vmax), groups = _hand_storms()
    g1 = climatology.CellGrid(*G1)
    for bad in (dict(lat=lat[:, :3]), dict(groups=groups[:4]), dict(groups=-groups - 1), dict(thresholds=(40.0, 25.0)),
                dict(thresholds=(nan,)), dict(vmax=np.where(np.isnan(vmax), 401.0, vmax)), dict(vmax=vmax - 100.0),
                dict(vmax=np.full_like(vmax, np.inf)), dict(n_groups=2)):
        kw = dict(lon=lon, lat=lat, vmax=vmax, groups=groups, thresholds=THR, n_groups=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            climatology.track_climatology(kw.pop('lon'), kw.pop('lat'), kw.pop('vmax'), kw.pop('groups'), g1, **kw)
    r = climatology.track_climatology(lon[:0], lat[:0], vmax[:0], groups[:0], g1, THR, n_groups=2)
    assert r['track'].shape == (2, 4, 12) and r['exceed'].shape == (2, 2, 4, 12) and r['genesis_k'].shape == (0,)
    for k in climatology.MAP_FIELDS:
        assert not r[k].any(), k
    # the ABI: bad grids, sizes and thresholds fail through tcr_last_error; a group out of range adds nothing to the maps
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        n_trk, n_t = lon.shape
        trk = _lib.HazardTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=lon.ctypes.data, lat=lat.ctypes.data, vmax=vmax.ctypes.data,
                                n_group=0, group_off=None)
        want = CN.climatology(lon, lat, vmax, [0, 1, 0, 1, 7, 2], 3, G1, THR)
        gi = np.array([0, 1, 0, 1, 7, 2], np.int32)
        res = {k: np.full(want[k].shape, 99, want[k].dtype) for k in want}
        out = _lib.ClimOut(**{k: v.ctypes.data for k, v in res.items()})
        thr = np.array(THR)

        def call(grid=G1, n_group=3, n_bin=2, tr=trk, t=thr):
            g = _lib.ClimGrid(lon0=grid[0], dlon=grid[1], nlon=grid[2], lat0=grid[3], dlat=grid[4], nlat=grid[5])
            return L.tcr_climatology_host(h, ctypes.byref(tr), gi.ctypes.data, n_group, ctypes.byref(g), n_bin,
                                          t.ctypes.data_as(_lib.DP), ctypes.byref(out))
        assert call() == 0
        _assert_equal(res, want)
        for kw in (dict(grid=(0.0, 30.0, 13, -60.0, 30.0, 4)), dict(grid=(0.0, 0.0, 12, -60.0, 30.0, 4)),
                   dict(grid=(nan, 30.0, 12, -60.0, 30.0, 4)), dict(grid=(0.0, 30.0, 12, -60.0, 30.0, 0)),
                   dict(grid=(0.0, 1e-3, 65536, 0.0, 1.0, 32768)), dict(n_group=0), dict(n_bin=65), dict(t=thr[::-1].copy()),
                   dict(tr=_lib.HazardTracks(n_trk=1 << 20, n_t=1 << 8, row_stride=1 << 8, lon=lon.ctypes.data, lat=lat.ctypes.data,
                                             vmax=vmax.ctypes.data))):
            assert call(**kw) == -1, kw
            assert b'tcr_climatology' in L.tcr_last_error(h), kw
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_end_to_end_run_downscaling_then_cli(golden_env, built_lib, tmp_path):
    import types
    from tropical_cyclone_risk_amd import compute, hazard, namelist
    nl = types.SimpleNamespace(**{k: getattr(namelist, k) for k in dir(namelist) if not k.startswith('__')})
    for k, v in dict(start_year=2001, end_year=2002, tracks_per_year=60, dataset_type='SYNTHETIC', output_directory=str(tmp_path),
                     exp_name='cl').items():
        setattr(nl, k, v)
    os.makedirs(tmp_path / 'cl', exist_ok=True)
    fn = compute.run_downscaling('NA', env=golden_env, nl=nl)
    for per_group in (False, True):
        out = str(tmp_path / ('clim_%d.npz' % per_group))
        cmd = [sys.executable, '-m', 'tropical_cyclone_risk_amd.climatology', fn, '--cells', '250:360:2,0:60:2', '--thresholds',
               '20,33', '--basin', 'NA', '--out', out] + (['--per-group'] if per_group else [])
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        assert 'seasonal cycle' in p.stdout
        z = np.load(out)
        assert set(z.files) == {'track', 'exceed', 'genesis', 'lmi', 'pdi', 'genesis_k', 'lmi_v', 'lmi_k', 'pdi_storm', 'n_storms',
                                'annual_pdi', 'seasonal_cycle', 'lmi_hist', 'thresholds', 'lmi_bins', 'lon_edges', 'lat_edges', 'cells',
                                'dt', 'q_scale', 'per_group', 'groups', 'group_file', 'group_year', 'basin', 'files'}
        lon, lat, vmax, groups, gfile, gyear, more = hazard.load_groups([fn], extra=('tc_month', 'tc_basins', 'time'))
        grid = climatology.CellGrid.from_bounds(250, 360, 0, 60, 2)
        mg, mn = (groups, 2) if per_group else (np.zeros_like(groups), 1)
        r = climatology.track_climatology(lon, lat, vmax, mg, grid, (20.0, 33.0), n_groups=mn)
        want = CN.climatology(lon, lat, vmax, mg, mn, (250.0, 2.0, 55, 0.0, 2.0, 30), (20.0, 33.0))
        _assert_equal(r, want)
        assert want['track'].sum() > 100
        for k in climatology.MAP_FIELDS:
            assert np.array_equal(z[k], r[k] if per_group else r[k][0]), k
        for k in climatology.STORM_FIELDS:
            assert np.array_equal(z[k], r[k], equal_nan=True), k
        dt = float(more['time'][0][1] - more['time'][0][0])
        assert float(z['dt']) == dt and z['group_year'].tolist() == [2001, 2002] and z['group_file'].tolist() == [0, 0]
        assert np.array_equal(z['n_storms'], np.bincount(groups, minlength=2))
        assert np.array_equal(z['annual_pdi'], climatology.annual_pdi(r['pdi_storm'], groups, dt, 2))
        assert np.array_equal(z['seasonal_cycle'], climatology.seasonal_cycle(more['tc_month'][0], more['tc_basins'][0], groups, 2,
                                                                              basin='NA'))
        assert z['seasonal_cycle'].sum() == lon.shape[0]
        assert np.array_equal(z['lmi_hist'], climatology.lmi_histogram(r['lmi_v'], groups, np.arange(0.0, 91.0, 5.0), 2))
