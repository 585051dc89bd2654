"""Landfall (tropical_cyclone_risk_amd/landfall.py, csrc/tcr_landfall.hip): the model's land decision taken on the nodes, the
sea -> land events of every storm, their exceedance counts, regions, return periods and site hazard.  CPU tests pin the NumPy
restatement to the reference's own `f_land.ev(lon, lat) == 1` and to a node-by-node evaluation, and check the host-side
aggregates, the CLI plumbing and the C struct layout; GPU tests (`-m gpu`) check the kernel against the restatement bit for bit."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import hazard_numpy as HN
from tests import landfall_numpy as LN
from tropical_cyclone_risk_amd import landfall

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
EVENT_KEYS = ('k', 'lon', 'lat', 'v_landfall', 'v_inland')


def _ref_land():
    return landfall.read_land(os.path.join(GOLDEN, 'ref_land.nc'))


def _fixture_points():
    z = np.load(os.path.join(GOLDEN, 'landfall_golden.npz'))
    tr = np.load(os.path.join(GOLDEN, 'tracks_NA_res0125.npz'))['traj']
    tx, ty = tr[:, 0].ravel(), tr[:, 1].ravel()
    live = ~np.isnan(tx) & ~np.isnan(ty)
    return z, np.concatenate([tx[live], z['px']]), np.concatenate([ty[live], z['py']])


def _toy_grid():
    """10-degree periodic globe: a continent (lon 100..150, lat 0..30) and an arctic island across the wrap (lon 350..30, lat 80)."""
    lon = np.arange(0.0, 360.0, 10.0)
    lat = np.arange(-80.0, 80.0 + 1e-9, 10.0)
    land = np.zeros((lat.size, lon.size))
    land[np.ix_((lat >= 0) & (lat <= 30), (lon >= 100) & (lon <= 150))] = 1
    land[-1, (lon >= 350) | (lon <= 30)] = 1
    return lon, lat, land


def _toy_tracks():
    nan = np.nan
    pts = [
        # sea, sea, gap, land (on a node), land, sea, land: two events
        [(90, 10), (95, 10), (nan, nan), (100, 10), (110, 15), (155, 10), (120, 20)],
        # genesis over land, sea, land: one event
        [(120, 10), (160, 10), (130, 10)],
        # the first track in the other longitude convention
        [(-270, 10), (-265, 10), (nan, nan), (-260, 10), (-250, 15), (-205, 10), (-240, 20)],
        # beyond the grid's last latitude (clamped) and across the wrap: (355, 85) is over the island
        [(340, 85), (355, 85), (-5, 88), (5, 89.9), (45, 85)],
        # a live sample with NaN lat is not live; lon above 360
        [(90, 10), (nan, 10), (460, 10), (465, 10), (470, 10)],
        [(nan, nan)] * 3,
    ]
    n_t = max(len(p) for p in pts)
    lon = np.full((len(pts), n_t), np.nan)
    lat = np.full((len(pts), n_t), np.nan)
    for s, p in enumerate(pts):
        for k, (x, y) in enumerate(p):
            lon[s, k], lat[s, k] = x, y
    vmax = 30.0 + np.arange(lon.size, dtype=float).reshape(lon.shape)
    vmax[2] = vmax[0]
    vmax[3, 0] = np.nan                                      # the last water sample before the island: NaN kept
    return lon, lat, vmax


def _stress_tracks(rng, grid, n_trk=600, n_t=150):
    """Random walks around coastlines of the 0.125-degree mask, with samples exactly on nodes and grid lines, NaN gaps and tails,
    both longitude conventions, longitudes above 360 and latitudes beyond the grid."""
    node = grid.land >= 1
    coast = node & ~(np.roll(node, 1, 1) & np.roll(node, -1, 1) & np.roll(node, 1, 0) & np.roll(node, -1, 0))
    j, i = np.nonzero(coast)
    s0 = rng.choice(j.size, n_trk)
    lon = grid.lon[i[s0]][:, None] + np.cumsum(rng.normal(0, 0.08, (n_trk, n_t)), axis=1)
    lat = grid.lat[j[s0]][:, None] + np.cumsum(rng.normal(0, 0.08, (n_trk, n_t)), axis=1)
    # snap a fifth of the samples to nodes, grid lines in lon or in lat
    snap = rng.random((n_trk, n_t))
    lon = np.where(snap < 0.1, np.round(lon * 8) / 8, lon)
    lat = np.where((snap < 0.05) | ((snap > 0.1) & (snap < 0.2)), np.round(lat * 8) / 8, lat)
    conv = rng.random(n_trk)
    lon[conv < 0.3] -= 360.0
    lon[conv > 0.9] += 360.0
    lat[:5] = np.linspace(88, 92, n_t)[None, :]              # beyond the last latitude
    lat[5:10] = np.linspace(-88, -92, n_t)[None, :]
    vmax = rng.uniform(0, 80, (n_trk, n_t))
    vmax[rng.random((n_trk, n_t)) < 0.05] = np.nan
    gap = rng.random((n_trk, n_t)) < 0.03
    lon[gap] = np.nan
    lat[rng.random((n_trk, n_t)) < 0.01] = np.nan
    end = rng.integers(1, n_t + 1, n_trk)
    tail = np.arange(n_t)[None, :] >= end[:, None]
    lon[tail] = lat[tail] = vmax[tail] = np.nan
    return lon, lat, vmax


def _assert_events_equal(got, want, flags=True):
    g = {k: np.asarray(v.cpu() if hasattr(v, 'cpu') else v) for k, v in got.items()}
    assert g['n_landfall'].dtype == np.int32 and np.array_equal(g['n_landfall'], want['n_landfall'])
    assert g['k'].dtype == np.int32 and g['k'].shape == want['k'].shape
    for k in EVENT_KEYS:
        a, b = g[k], want[k]
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)           # bit for bit, NaN included
        assert np.array_equal(a, b), k
    if flags:
        assert g['flags'].dtype == np.uint8 and np.array_equal(g['flags'], want['flags'])


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_restatement_equals_node_by_node_rule():
    rng = np.random.default_rng(4)
    lon, lat, land = _toy_grid()
    land[5, 7] = np.nan                                      # NaN node: water
    x = np.concatenate([rng.uniform(-400, 760, 400), np.repeat(lon, 3), rng.choice(lon, 100) + 360.0, [355.0, 359.999, -0.0, np.inf]])
    y = np.concatenate([rng.uniform(-95, 95, 400), rng.choice(lat, lon.size * 3), rng.uniform(-10, 40, 100), [85.0, 80.0, 80.0, 10.0]])
    assert LN.periodic(lon)
    assert np.array_equal(LN.over_land(x, y, lon, lat, land), LN.brute_force_over_land(x, y, lon, lat, land))
    # a regional (not periodic) grid clamps on both axes
    rl, rla = lon[8:20], lat[6:12]
    rland = land[6:12, 8:20]
    assert not LN.periodic(rl)
    xr = np.concatenate([rng.uniform(60, 210, 300), np.repeat(rl, 4)])
    yr = np.concatenate([rng.uniform(-30, 50, 300), rng.choice(rla, rl.size * 4)])
    assert np.array_equal(LN.over_land(xr, yr, rl, rla, rland), LN.brute_force_over_land(xr, yr, rl, rla, rland))
    assert LN.over_land(xr, yr, rl, rla, rland).sum() > 30


def test_restatement_equals_the_reference_decision_outside_the_flicker_band():
    grid = _ref_land()
    assert grid.periodic and grid.land.shape == (1440, 2880)
    z, x, y = _fixture_points()
    ol = LN.over_land(x, y, grid.lon, grid.lat, grid.land)
    for b in ('NA', 'GL'):
        ev = np.concatenate([z['ev_track_%s' % b], z['ev_%s' % b]])
        c = z['crop_%s' % b]
        keep = (x >= c[0]) & (x <= c[1]) & (y >= c[2]) & (y <= c[3])      # outside the crop the reference clamps, the contract wraps
        band = (ev >= 1 - 1e-12) & (ev < 1)
        bad = keep & ~band & (ol != (ev == 1))
        assert not bad.any(), (b, int(bad.sum()), x[bad][:5], y[bad][:5], ev[bad][:5], 'flicker band: %d' % int((keep & band).sum()))
        assert (ol[keep & band]).all(), (b, 'flicker band points must be land', int((keep & band).sum()))
        assert keep.sum() > 5000 and (keep & (ev == 1)).sum() > 500
        print('%s: %d points compared, %d in the flicker band 1 - 1e-12 <= ev < 1 (all land here)'
              % (b, int(keep.sum()), int((keep & band).sum())))


def test_hand_built_events():
    lon, lat, land = _toy_grid()
    tl, ta, vm = _toy_tracks()
    r = LN.landfalls(tl, ta, vm, lon, lat, land)
    assert r['n_landfall'].tolist() == [2, 1, 2, 1, 1, 0]
    assert r['k'][0].tolist() == [3, 6] and r['v_landfall'][0].tolist() == [vm[0, 1], vm[0, 5]]
    assert r['v_inland'][0].tolist() == [vm[0, 3], vm[0, 6]]
    assert r['lon'][0].tolist() == [100.0, 120.0] and r['lat'][0].tolist() == [10.0, 20.0]
    assert r['k'][1].tolist() == [2, -1] and r['v_landfall'][1, 0] == vm[1, 1]
    for k in EVENT_KEYS[1:]:                                 # the other convention: the same events, its own coordinates
        same = np.array_equal(r[k][2], r[k][0], equal_nan=True)
        assert same == (k != 'lon'), k
    assert np.array_equal(r['lon'][2], r['lon'][0] - 360.0)
    assert r['k'][3].tolist() == [1, -1] and np.isnan(r['v_landfall'][3, 0]) and r['v_inland'][3, 0] == vm[3, 1]
    assert r['k'][4].tolist() == [2, -1] and r['v_landfall'][4, 0] == vm[4, 0]      # lat NaN at 1: not live
    assert r['flags'][0].tolist() == [0, 0, 2, 1, 1, 0, 1] and r['flags'][5].tolist() == [2] * 7
    assert r['flags'][3].tolist()[:5] == [0, 1, 1, 1, 0]


def test_counts_regions_and_return_periods_by_hand():
    from tropical_cyclone_risk_amd import hazard
    nan = np.nan
    ev = dict(k=np.array([[3, 9], [4, -1], [-1, -1], [2, 5]], np.int32),
              lon=np.array([[280.0, 120.0], [-80.0, nan], [nan, nan], [179.0, -179.5]]),
              lat=np.array([[25.0, 20.0], [30.0, nan], [nan, nan], [10.0, 12.0]]),
              v_landfall=np.array([[40.0, 60.0], [nan, nan], [nan, nan], [20.0, 35.0]]))
    groups = np.array([0, 1, 0, 2])
    c = landfall.landfall_counts(ev, groups, [30.0, 50.0], n_groups=4,
                                 regions={'US': (-100.0, -60.0, 20.0, 35.0), 'DL': (170.0, -170.0, 0.0, 15.0), 'NONE': (0, 1, 0, 1)})
    assert c['first'].tolist() == [[1, 0], [0, 0], [0, 0], [0, 0]]
    assert c['max'].tolist() == [[1, 1], [0, 0], [1, 0], [0, 0]]
    assert c['n_storms'].tolist() == [1, 1, 1, 0]            # a NaN intensity still makes a landfalling storm
    assert c['region_names'].tolist() == ['US', 'DL', 'NONE']
    us, dl, none = 0, 1, 2
    assert c['region_first'][us].tolist() == [[1, 0], [0, 0], [0, 0], [0, 0]]
    assert c['region_n_storms'][us].tolist() == [1, 1, 0, 0]
    assert c['region_first'][dl].tolist() == [[0, 0], [0, 0], [0, 0], [0, 0]]        # first event in the box: 20 m/s
    assert c['region_max'][dl].tolist() == [[0, 0], [0, 0], [1, 0], [0, 0]]
    assert c['region_n_storms'][dl].tolist() == [0, 0, 1, 0]
    assert c['region_n_storms'][none].sum() == 0
    rp = hazard.return_periods(c['max'][None], 4)[0]
    assert rp.tolist() == [2.0, 4.0]
    assert np.isinf(hazard.return_periods(c['region_first'], 4)[dl]).all()
    assert landfall.in_box([359.0, -1.0, 1.0, 3.0], [0, 0, 0, 0], (-2.0, 2.0, -1, 1)).tolist() == [True, True, True, False]
    assert landfall.in_box([nan, 10.0], [0.0, nan], (0, 360, -90, 90)).tolist() == [False, False]


def test_cli_parsing():
    a = landfall.parse_args(['x.nc', 'y.nc', '--land', 'land.nc', '--region', 'FL=-88:-79,24:31', '--region=DL=170:-170,0:15',
                             '--site=-80.19,25.76', '--thresholds', '20:60:10', '--radius-km', '50'])
    assert a.tracks == ['x.nc', 'y.nc'] and a.land == 'land.nc' and a.radius_km == 50.0
    assert a.region == [('FL', (-88.0, -79.0, 24.0, 31.0)), ('DL', (170.0, -170.0, 0.0, 15.0))]
    assert np.array_equal(a.thresholds, [20, 30, 40, 50, 60]) and a.out == 'landfall.npz'
    b = landfall.parse_args(['x.nc', '--land', 'l.nc'])
    assert b.region == [] and np.array_equal(b.thresholds, landfall.DEFAULT_THRESHOLDS)
    from tropical_cyclone_risk_amd import hazard
    assert hazard.collect_sites(b)[0].size == 0
    for bad in (['x.nc'], ['x.nc', '--land', 'l.nc', '--region', 'FL=1:2'], ['x.nc', '--land', 'l.nc', '--region', 'FL=1:2,5:4'],
                ['x.nc', '--land', 'l.nc', '--region', '=1:2,3:4']):
        with pytest.raises(SystemExit):
            landfall.parse_args(bad)


def test_read_land_flips_a_north_to_south_grid(tmp_path):
    from scipy.io import netcdf_file
    lon, lat, land = _toy_grid()
    fn = str(tmp_path / 'land.nc')
    with netcdf_file(fn, 'w', version=2) as f:
        f.createDimension('lat', lat.size); f.createDimension('lon', lon.size)
        for name, arr, dims in (('lat', lat[::-1], ('lat',)), ('lon', lon, ('lon',)), ('land', land[::-1], ('lat', 'lon'))):
            v = f.createVariable(name, 'd', dims)
            v[:] = arr
    g = landfall.read_land(fn)
    assert np.array_equal(g.lat, lat) and np.array_equal(g.land, land) and g.periodic
    assert not landfall.LandGrid(lon[:10], lat, land[:, :10]).periodic
    with pytest.raises(ValueError):
        landfall.LandGrid(lon, lat, land[:, :5])


def test_land_struct_layout_matches_header():
    from tropical_cyclone_risk_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tcrisk_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
           'sizeof(tcr_land_grid),offsetof(tcr_land_grid, nlat),offsetof(tcr_land_grid, lon),'
           'offsetof(tcr_land_grid, lat),offsetof(tcr_land_grid, land));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'sz.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 'sz')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    G = _lib.LandGrid
    assert sizes == [ctypes.sizeof(G), G.nlat.offset, G.lon.offset, G.lat.offset, G.land.offset]


def test_landfall_symbols_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_land_upload', 'tcr_land_info', 'tcr_landfall_dev', 'tcr_landfall_host'):
        assert hasattr(L, name), name


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_matches_restatement_on_the_reference_mask(built_lib):
    grid = _ref_land()
    lon, lat, vmax = _stress_tracks(np.random.default_rng(8), grid)
    want = LN.landfalls(lon, lat, vmax, grid.lon, grid.lat, grid.land)
    got = landfall.detect_landfalls(lon, lat, vmax, grid, return_flags=True)
    _assert_events_equal(got, want)
    assert (want['n_landfall'] > 0).sum() > 100 and want['n_landfall'].max() > 8    # the rerun with a larger capacity ran
    # the fixture's points (the reference's own decisions pinned the restatement to them), as tracks of 97 samples
    _, x, y = _fixture_points()
    n = x.size // 97 * 97
    fx, fy = x[:n].reshape(-1, 97), y[:n].reshape(-1, 97)
    fv = np.arange(n, dtype=float).reshape(fx.shape)
    want = LN.landfalls(fx, fy, fv, grid.lon, grid.lat, grid.land)
    _assert_events_equal(landfall.detect_landfalls(fx, fy, fv, grid, return_flags=True), want)
    assert want['n_landfall'].sum() > 500


@pytest.mark.gpu
def test_gpu_hand_built_events_and_a_grid_beyond_lds(built_lib):
    from tropical_cyclone_risk_amd import _lib
    lon, lat, land = _toy_grid()
    tl, ta, vm = _toy_tracks()
    _assert_events_equal(landfall.detect_landfalls(tl, ta, vm, (lon, lat, land), return_flags=True),
                         LN.landfalls(tl, ta, vm, lon, lat, land))
    # a regional 9000 x 400 grid: node coordinates do not fit the kernel's LDS copy and are read from global memory
    rng = np.random.default_rng(2)
    glon = 260.0 + 0.01 * np.arange(9000)
    glat = 0.1 * np.arange(400)
    gland = (rng.random((400, 9000)) < 0.6).astype(float)
    gland[rng.random(gland.shape) < 0.01] = np.nan
    gl = np.clip(255.0 + np.cumsum(rng.normal(0.3, 0.05, (200, 400)), axis=1) * 0.3 + rng.uniform(0, 30, (200, 1)), 200, 400)
    ga = rng.uniform(-2, 42, (200, 1)) + np.cumsum(rng.normal(0, 0.05, (200, 400)), axis=1)
    gl[:, ::7] = np.round(gl[:, ::7] * 100) / 100
    gv = rng.uniform(0, 80, gl.shape)
    want = LN.landfalls(gl, ga, gv, glon, glat, gland)
    _assert_events_equal(landfall.detect_landfalls(gl, ga, gv, (glon, glat, gland), return_flags=True), want)
    assert want['n_landfall'].sum() > 1000
    # the library derives the periodic flag
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        for g, per in ((_ref_land(), 1), (landfall.LandGrid(glon, glat, gland), 0)):
            s = _lib.LandGrid(nlon=g.lon.size, nlat=g.lat.size, lon=g.lon.ctypes.data, lat=g.lat.ctypes.data, land=g.land.ctypes.data)
            assert L.tcr_land_upload(h, ctypes.byref(s)) == 0
            a, b, p = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
            assert L.tcr_land_info(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(p)) == 0
            assert (a.value, b.value, p.value) == (g.lon.size, g.lat.size, per)
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_device_tensors_on_a_side_stream(built_lib):
    import torch
    from tropical_cyclone_risk_amd.engine import TCEngine
    grid = _ref_land()
    lon, lat, vmax = _stress_tracks(np.random.default_rng(21), grid, n_trk=300)
    want = LN.landfalls(lon, lat, vmax, grid.lon, grid.lat, grid.land)
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(a, device=dev) for a in (lon, lat, vmax)]
    eng = TCEngine('NA', device=0)
    side = torch.cuda.Stream(dev)
    try:
        for _ in range(2):                                   # the second call reuses the engine's uploaded grid
            with torch.cuda.stream(side):
                r = landfall.detect_landfalls(*t, grid, engine=eng, return_flags=True)
            side.synchronize()
            assert all(v.device == dev for v in r.values())
            _assert_events_equal(r, want)
        with torch.cuda.stream(side):
            s = landfall.landfall_site_hazard(r, np.zeros(lon.shape[0], np.int64), torch.tensor([280.0], device=dev),
                                              torch.tensor([25.0], device=dev), engine=eng)
        side.synchronize()
        assert s['counts'].device == dev
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_bad_arguments_raise(built_lib):
    from tropical_cyclone_risk_amd import _lib
    lon, lat, land = _toy_grid()
    tl, ta, vm = _toy_tracks()
    with pytest.raises(_lib.TcrError):                       # unsorted grid
        landfall.detect_landfalls(tl, ta, vm, (lon[::-1].copy(), lat, land))
    with pytest.raises(_lib.TcrError):                       # repeated node
        landfall.detect_landfalls(tl, ta, vm, (np.concatenate([[0.0], lon[:-1]]), lat, land))
    with pytest.raises(ValueError):
        landfall.detect_landfalls(tl, ta[:, :3], vm, (lon, lat, land))
    with pytest.raises(ValueError):
        landfall.detect_landfalls(tl, ta, vm, (lon, lat, land[:, :4]))
    r = landfall.detect_landfalls(tl[:0], ta[:0], vm[:0], (lon, lat, land), return_flags=True)
    assert r['n_landfall'].shape == (0,) and r['k'].shape == (0, 0) and r['flags'].shape == (0, tl.shape[1])
    # the ABI: no grid uploaded, negative capacity
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        trk = _lib.HazardTracks(n_trk=tl.shape[0], n_t=tl.shape[1], row_stride=tl.shape[1], lon=tl.ctypes.data, lat=ta.ctypes.data,
                                vmax=vm.ctypes.data, n_group=0, group_off=None)
        n = np.zeros(tl.shape[0], np.int32)
        assert L.tcr_landfall_host(h, ctypes.byref(trk), 0, n.ctypes.data, None, None, None, None, None, None) == -1
        assert b'tcr_land_upload' in L.tcr_last_error(h)
        g = _lib.LandGrid(nlon=lon.size, nlat=lat.size, lon=lon.ctypes.data, lat=lat.ctypes.data, land=land.ctypes.data)
        assert L.tcr_land_upload(h, ctypes.byref(g)) == 0
        assert L.tcr_landfall_host(h, ctypes.byref(trk), -1, n.ctypes.data, None, None, None, None, None, None) == -1
        assert L.tcr_landfall_host(h, ctypes.byref(trk), 0, n.ctypes.data, None, None, None, None, None, None) == 0
        assert n.tolist() == [2, 1, 2, 1, 1, 0]             # counts only
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_site_stage_matches_hazard_restatement(built_lib):
    grid = _ref_land()
    lon, lat, vmax = _stress_tracks(np.random.default_rng(3), grid, n_trk=400)
    ev = landfall.detect_landfalls(lon, lat, vmax, grid)
    groups = np.random.default_rng(1).integers(0, 3, lon.shape[0])
    live = np.argwhere(ev['k'] >= 0)[::7][:40]
    slon = np.concatenate([ev['lon'][live[:, 0], live[:, 1]] + 0.3, [280.0, -80.0]])
    slat = np.concatenate([ev['lat'][live[:, 0], live[:, 1]] - 0.2, [25.0, 25.0]])
    thr = np.arange(10, 81, 10).astype(float)
    r = landfall.landfall_site_hazard(ev, groups, slon, slat, radius_km=150.0, thresholds=thr, return_max=True, n_groups=3)
    m, amb = HN.site_max(ev['lon'], ev['lat'], ev['v_landfall'], slon, slat, 150.0)
    assert not amb.any()
    assert np.array_equal(r['site_max'].view(np.int64), m.view(np.int64))
    assert np.array_equal(r['counts'], HN.counts(m, groups, 3, thr)) and r['counts'].sum() > 20


@pytest.mark.gpu
def test_gpu_end_to_end_run_downscaling_then_cli(golden_env, built_lib, tmp_path):
    import types
    from tropical_cyclone_risk_amd import compute, fields, hazard, io as tio, namelist
    nl = types.SimpleNamespace(**{k: getattr(namelist, k) for k in dir(namelist) if not k.startswith('__')})
    for k, v in dict(start_year=2001, end_year=2002, tracks_per_year=60, dataset_type='SYNTHETIC', output_directory=str(tmp_path),
                     exp_name='lf').items():
        setattr(nl, k, v)
    os.makedirs(tmp_path / 'lf', exist_ok=True)
    fn = compute.run_downscaling('NA', env=golden_env, nl=nl)
    files = fields.write_reference_files(golden_env, str(tmp_path / 'env'), 2001)
    out = str(tmp_path / 'landfall.npz')
    cmd = [sys.executable, '-m', 'tropical_cyclone_risk_amd.landfall', fn, '--land', files['land'], '--out', out,
           '--region', 'GULF=-98:-80,18:31', '--region', 'ALL=0:360,-90:90', '--site=-80.1918,25.7617', '--thresholds', '10:80:5']
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert 'return period' in p.stdout
    z = np.load(out)
    assert set(z.files) == {'n_landfall', 'event_k', 'thresholds', 'groups', 'total_years', 'group_file', 'group_year', 'files',
                            'counts_first', 'counts_max', 'n_storms', 'return_period_first', 'return_period_max', 'region_names',
                            'region_box', 'region_counts_first', 'region_counts_max', 'region_n_storms',
                            'region_return_period_first', 'region_return_period_max', 'event_lon', 'event_lat', 'event_v_landfall',
                            'event_v_inland', 'site_lon', 'site_lat', 'radius_km', 'site_counts', 'site_return_period'}
    # the in-process API on the same inputs
    lon, lat, vmax, groups, gfile, gyear = hazard.load_groups([fn])
    grid = landfall.read_land(files['land'])
    ev = landfall.detect_landfalls(lon, lat, vmax, grid)
    assert (ev['n_landfall'] > 0).any(), 'no storm made landfall'
    want = LN.landfalls(lon, lat, vmax, grid.lon, grid.lat, grid.land)
    _assert_events_equal(ev, want, flags=False)
    assert np.array_equal(z['n_landfall'], ev['n_landfall']) and np.array_equal(z['event_k'], ev['k'])
    for k in landfall.EVENT_FIELDS:
        assert np.array_equal(z['event_' + k], ev[k], equal_nan=True), k
    c = landfall.landfall_counts(ev, groups, np.arange(10, 81, 5), regions=[('GULF', (-98, -80, 18, 31)), ('ALL', (0, 360, -90, 90))],
                                 n_groups=2)
    assert int(z['total_years']) == 2 and z['group_year'].tolist() == [2001, 2002]
    for a, b in (('counts_first', 'first'), ('counts_max', 'max'), ('n_storms', 'n_storms'), ('region_counts_first', 'region_first'),
                 ('region_counts_max', 'region_max'), ('region_n_storms', 'region_n_storms')):
        assert np.array_equal(z[a], c[b]), a
    assert np.array_equal(z['region_counts_max'][1], c['max'])          # the whole globe is the basin
    assert np.array_equal(z['return_period_first'], hazard.return_periods(c['first'][None], 2)[0])
    s = landfall.landfall_site_hazard(ev, groups, [-80.1918], [25.7617], thresholds=np.arange(10, 81, 5), n_groups=2)
    assert np.array_equal(z['site_counts'], s['counts'])
