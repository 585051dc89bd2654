"""Throughput of the site-hazard kernels (csrc/tcr_hazard.hip) on two workloads, against NumPy on a subsample:

  coast  10^4 coast-like sites (a jittered Gulf / US East coast polyline) x 45 000 tracks (45 years x 1 000) x 361 samples
  grid   the 0.25-degree NA grid (lon 260..350, lat 0..60: 361 x 241 = 87 001 sites) x the same tracks

Tracks are seeded random walks (genesis 8-25 N, 280-340 E, drifting west then recurving north-east, 5 % NaN vmax holes, NaN
tails after 80-361 samples).  Reports ms per call (device events, median of 3 after a warm-up), pairs/s counted two ways
(raw: sites x live samples; evaluated: the (site, sample) distance tests left after culling, tcr_hazard_pairs), and NumPy (the
notebook's haversine + where + nanmax, tests/hazard_numpy.py) on a few sites, extrapolated to the same raw work.  The GPU result
on those sites is checked against NumPy.

    python tools/bench_hazard.py [--quick]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tests import hazard_numpy as HN  # noqa: E402
from tropical_cyclone_risk_amd import _lib, hazard  # noqa: E402

R_KM = 100.0
THR = np.arange(10, 81, 5).astype(np.float64)


def make_tracks(rng, n_years, per_year, n_t=361):
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


def coast_sites(rng, n):
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
    glon, glat = np.meshgrid(np.arange(260.0, 350.0 + 1e-9, 0.25), np.arange(0.0, 60.0 + 1e-9, 0.25))
    return glon.ravel(), glat.ravel()


def run_gpu(L, h, dt, groups, slon, slat, K=3):
    dev = dt[0].device
    n_trk, n_t = dt[0].shape
    n_groups = int(groups.max()) + 1
    group_off = np.zeros(n_groups + 1, np.int64)
    group_off[1:] = np.cumsum(np.bincount(groups, minlength=n_groups))
    order = hazard._spatial_order(torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev), torch)
    sl, sa = torch.as_tensor(slon, device=dev)[order].contiguous(), torch.as_tensor(slat, device=dev)[order].contiguous()
    counts = torch.empty((len(slon), n_groups, THR.size), dtype=torch.int32, device=dev)
    trk = _lib.HazardTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=dt[0].data_ptr(), lat=dt[1].data_ptr(), vmax=dt[2].data_ptr(),
                            n_group=n_groups, group_off=group_off.ctypes.data_as(C.POINTER(C.c_int64)))
    st = torch.cuda.current_stream(dev)

    def launch():
        if L.tcr_hazard_dev(h, C.byref(trk), len(slon), sl.data_ptr(), sa.data_ptr(), R_KM, THR.size, THR.ctypes.data_as(_lib.DP),
                            counts.data_ptr(), None, C.c_void_p(st.cuda_stream)) != 0:
            raise _lib.TcrError(L.tcr_last_error(h).decode())
    launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(K):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); launch(); e1.record(st)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    pairs = C.c_int64()
    if L.tcr_hazard_pairs(h, C.byref(pairs)) != 0:
        raise _lib.TcrError(L.tcr_last_error(h).decode())
    out = torch.empty_like(counts)
    out[order] = counts
    return float(np.median(ms)), ms, int(pairs.value), out.cpu().numpy()


def numpy_check(lon, lat, vmax, groups, slon, slat, gpu_counts, dt, idx):
    """NumPy on the sites `idx`: time per site (the notebook's computation) and equality with the GPU."""
    n_groups = int(groups.max()) + 1
    t = 0.0
    for i in idx:
        t0 = time.perf_counter()
        m, amb = HN.site_max(lon, lat, vmax, slon[i:i + 1], slat[i:i + 1], R_KM)
        t += time.perf_counter() - t0
        assert not amb.any(), 'ambiguous pair in the subsample'
        assert np.array_equal(gpu_counts[i], HN.counts(m, groups, n_groups, THR)[0]), ('counts differ at site', int(i))
    r = hazard.site_hazard(dt[0], dt[1], dt[2], groups, torch.as_tensor(slon[idx], device=dt[0].device),
                           torch.as_tensor(slat[idx], device=dt[0].device), radius_km=R_KM, thresholds=THR, return_max=True)
    gm = r['site_max'].cpu().numpy()
    for k, i in enumerate(idx):
        m, _ = HN.site_max(lon, lat, vmax, slon[i:i + 1], slat[i:i + 1], R_KM)
        assert np.array_equal(gm[k:k + 1].view(np.int64), m.view(np.int64)), ('site_max differs at site', int(i))
    return t / len(idx)


def main():
    quick = '--quick' in sys.argv
    rng = np.random.default_rng(7)
    n_years, per_year = (5, 200) if quick else (45, 1000)
    lon, lat, vmax, groups = make_tracks(rng, n_years, per_year)
    live = int((~np.isnan(lon)).sum())
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in (lon, lat, vmax)]
    L = _lib.lib()
    h = C.c_void_p()
    if L.tcr_ctx_create(0, C.byref(h)) != 0:
        raise _lib.TcrError(L.tcr_last_error(None).decode())
    results = []
    try:
        for name, (slon, slat) in (('coast', coast_sites(rng, 1000 if quick else 10000)), ('grid', grid_sites())):
            ms, all_ms, pairs, counts = run_gpu(L, h, dt, groups, slon, slat)
            raw = len(slon) * live
            idx = np.sort(np.random.default_rng(1).choice(len(slon), 4, replace=False))
            # the subsample includes sites that do see storms
            hit = np.nonzero(counts.sum(axis=(1, 2)))[0]
            if len(hit):
                idx = np.unique(np.concatenate([idx, hit[np.linspace(0, len(hit) - 1, 4).astype(int)]]))
            np_s_per_site = numpy_check(lon, lat, vmax, groups, slon, slat, counts, dt, idx)
            np_rate = live / np_s_per_site
            np_total_s = np_s_per_site * len(slon)
            row = dict(workload=name, sites=len(slon), tracks=lon.shape[0], samples=lon.shape[1], live_samples=live,
                       gpu_ms=round(ms, 3), gpu_ms_runs=[round(x, 3) for x in all_ms], raw_pairs=raw, evaluated_pairs=pairs,
                       culled_fraction=round(1 - pairs / raw, 5), raw_pairs_per_s=raw / (ms / 1e3),
                       evaluated_pairs_per_s=pairs / (ms / 1e3), numpy_pairs_per_s=np_rate, numpy_sites_checked=len(idx),
                       numpy_extrapolated_s=round(np_total_s, 1), speedup=round(np_total_s / (ms / 1e3), 1),
                       sites_with_counts=int((counts.sum(axis=(1, 2)) > 0).sum()), check='gpu == numpy on the subsample')
            results.append(row)
            print(json.dumps(row), flush=True)
    finally:
        L.tcr_ctx_destroy(h)
    for r in results:
        print('%-5s %6d sites: %9.2f ms  raw %.3g pairs/s, evaluated %.3g pairs/s (%.2f %% culled); NumPy %.3g pairs/s '
              '-> %.0f s extrapolated, speed-up %.0fx' % (r['workload'], r['sites'], r['gpu_ms'], r['raw_pairs_per_s'],
                                                       r['evaluated_pairs_per_s'], 100 * r['culled_fraction'],
                                                       r['numpy_pairs_per_s'], r['numpy_extrapolated_s'], r['speedup']))


if __name__ == '__main__':
    main()
