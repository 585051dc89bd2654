"""What the analysis bench tools (bench_hazard, bench_landfall, bench_climatology, bench_windfield, bench_loss) share: the seeded
workloads (every tool draws from its generator in the order of its docstring), a library context, device-event timing, and the
tracks structs and the timed site scan on device tensors."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tropical_cyclone_risk_amd import _lib, sitescan  # noqa: E402

R_KM = 100.0
THR = np.arange(10, 81, 5).astype(np.float64)


def sizes(quick):
    """(years, tracks per year, coast sites) of the full and the --quick workload."""
    return (5, 200, 1000) if quick else (45, 1000, 10000)


def make_tracks(rng, n_years, per_year, n_t=361):
    """Seeded random walks: genesis 8-25 N, 280-340 E, drifting west then recurving north-east, 5 % NaN vmax holes, NaN tails
    after 80-361 samples; one group per year."""
    n = n_years * per_year
    lon = np.empty((n, n_t)); lat = np.empty((n, n_t))
    lon[:, 0] = rng.uniform(280, 340, n); lat[:, 0] = rng.uniform(8, 25, n)
    u = -0.25 + 0.004 * np.arange(n_t)[None, :] * rng.uniform(0.3, 1.0, (n, 1))      # westward, recurving
    lon[:, 1:] = lon[:, :1] + np.cumsum(np.clip(u[:, 1:], -0.4, 0.4) + rng.normal(0, 0.05, (n, n_t - 1)), axis=1)
    lat[:, 1:] = lat[:, :1] + np.cumsum(0.05 + rng.normal(0, 0.05, (n, n_t - 1)), axis=1)
    lat = np.clip(lat, -89, 89)
    vmax = np.clip(20 + np.cumsum(rng.normal(0.1, 1.0, (n, n_t)), axis=1), 0, 90)
    vmax[rng.random((n, n_t)) < 0.05] = np.nan
    end = rng.integers(80, n_t + 1, n)
    tail = np.arange(n_t)[None, :] >= end[:, None]
    lon[tail] = lat[tail] = vmax[tail] = np.nan
    groups = np.repeat(np.arange(n_years), per_year)
    return lon, lat, vmax, groups


def make_storms(rng, n_years, per_year):
    """make_tracks' walks with v a bounded random walk in 15-75 m/s and env winds of N(0, 8 m/s)."""
    lon, lat, _, groups = make_tracks(rng, n_years, per_year)
    n, n_t = lon.shape
    v = np.clip(35 + np.cumsum(rng.normal(0.0, 1.0, (n, n_t)), axis=1), 15, 75)
    env = [rng.normal(0, 8, (n, n_t)) for _ in range(4)]
    tail = np.isnan(lon)
    v[tail] = np.nan
    for e in env:
        e[tail] = np.nan
    return lon, lat, v, env, groups


def coast_sites(rng, n):
    """n coast-like sites: a jittered Gulf / US East coast polyline."""
    pts = np.array([[262.5, 18.0], [262.5, 25.5], [266.0, 29.5], [271.0, 30.3], [276.5, 30.0], [277.5, 27.0], [279.8, 25.3],
                    [280.0, 27.0], [278.8, 30.5], [281.0, 32.0], [284.5, 35.2], [286.0, 38.5], [288.0, 41.3], [290.0, 42.0],
                    [294.0, 44.0], [300.0, 46.5]])
    seg = np.linalg.norm(np.diff(pts, axis=0), axis=1)
    s = np.sort(rng.uniform(0, seg.sum(), n))
    k = np.searchsorted(np.cumsum(seg), s, side='right').clip(0, len(seg) - 1)
    f = (s - np.concatenate([[0], np.cumsum(seg)])[k]) / seg[k]
    p = pts[k] + f[:, None] * (pts[k + 1] - pts[k]) + rng.normal(0, 0.05, (n, 2))
    lon = np.where(rng.random(n) < 0.5, p[:, 0] - 360.0, p[:, 0])          # both longitude conventions
    return lon, p[:, 1]


def grid_sites():
    """The 0.25-degree NA grid (lon 260..350, lat 0..60: 361 x 241 = 87 001 sites)."""
    glon, glat = np.meshgrid(np.arange(260.0, 350.0 + 1e-9, 0.25), np.arange(0.0, 60.0 + 1e-9, 0.25))
    return glon.ravel(), glat.ravel()


def check(L, h, rc):
    if rc != 0:
        raise _lib.TcrError(L.tcr_last_error(h).decode())


@contextlib.contextmanager
def open_context(L=None):
    """(library, context on device 0); L: a library other than the tree's own."""
    L = L or _lib.lib()
    h = C.c_void_p()
    check(L, None, L.tcr_ctx_create(0, C.byref(h)))
    try:
        yield L, h
    finally:
        L.tcr_ctx_destroy(h)


def timed(fn, stream, K=3):
    """(median, runs) in ms by device events on `stream`, K runs after a warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(K):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), ms


def group_offsets(groups):
    """(n_groups, group_off [n_groups + 1]) of sorted groups."""
    n_groups = int(groups.max()) + 1
    group_off = np.zeros(n_groups + 1, np.int64)
    group_off[1:] = np.cumsum(np.bincount(groups, minlength=n_groups))
    return n_groups, group_off


def _tracks(struct, names, dt, groups, **more):
    n_trk, n_t = dt[0].shape
    n_groups, group_off = group_offsets(groups) if groups is not None else (0, None)
    trk = struct(n_trk=n_trk, n_t=n_t, row_stride=n_t, n_group=n_groups,
                 group_off=None if group_off is None else group_off.ctypes.data_as(C.POINTER(C.c_int64)),
                 **{k: a.data_ptr() for k, a in zip(names, dt)}, **more)
    trk.keep = (dt, group_off)
    return trk


def hazard_tracks(dt, groups=None):
    """tcr_hazard_tracks of the device tensors (lon, lat, vmax); groups: sorted (None: an analysis without groups)."""
    return _tracks(_lib.HazardTracks, ('lon', 'lat', 'vmax'), dt, groups)


def wind_tracks(dt, groups):
    """tcr_wind_tracks of the device tensors (lon, lat, v, u250, v250, u850, v850), rm modelled; groups: sorted."""
    return _tracks(_lib.WindTracks, ('lon', 'lat', 'v', 'u250', 'v250', 'u850', 'v850'), dt, groups, rmax_km=None)


def time_site_scan(L, h, entry, trk, before, after, slon, slat, K=3):
    """Times L.<entry>_dev(h, trk, *before, sites in spatial order, *after, THR, counts, no site_max) on the current stream of
    the tracks' device: (median ms, runs, the evaluated pairs of <entry>_pairs, counts in the caller's site order)."""
    dev = trk.keep[0][0].device
    tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
    order = sitescan.spatial_order(tl, ta, torch)
    sl, sa = tl[order].contiguous(), ta[order].contiguous()
    counts = torch.empty((len(slon), trk.n_group, THR.size), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)
    fn = getattr(L, entry + '_dev')

    def launch():
        check(L, h, fn(h, C.byref(trk), *before, len(slon), sl.data_ptr(), sa.data_ptr(), *after, THR.size, THR.ctypes.data_as(_lib.DP),
                       counts.data_ptr(), None, C.c_void_p(st.cuda_stream)))
    ms, runs = timed(launch, st, K)
    pairs = C.c_int64()
    check(L, h, getattr(L, entry + '_pairs')(h, C.byref(pairs)))
    out = torch.empty_like(counts)
    out[order] = counts
    return ms, runs, int(pairs.value), out.cpu().numpy()
