"""Throughput of the wind-footprint kernels (csrc/tcr_windfield.hip) on two site sets, against the NumPy restatement on a subsample:

  coast  10^4 coast-like sites (tools/bench_hazard.py's jittered Gulf / US East coast polyline) x 45 000 tracks (45 years x 1 000)
         x 361 samples
  grid   the 0.25-degree NA grid (lon 260..350, lat 0..60: 361 x 241 = 87 001 sites) x the same tracks

Tracks are bench_hazard's seeded random walks (NaN tails after 80-361 samples) with v a bounded random walk in 15-75 m/s and
env winds of N(0, 8 m/s).  r_out = 500 km, substeps 1 and 4, c = 1, rm modelled.  Reports ms per call (device events, median of 3
after a warm-up), the raw pairs (sites x samples and sub-samples), the evaluated pairs left after culling (tcr_windfield_pairs)
and the culled fraction, evaluated pairs/s, and the restatement (tests/windfield_numpy.py) on a few sites on one core,
extrapolated to all sites; the GPU result on those sites is checked against it.

    python tools/bench_windfield.py [--quick]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402
from bench_hazard import coast_sites, grid_sites, make_tracks  # noqa: E402
from tests import windfield_numpy as WN  # noqa: E402
from tropical_cyclone_risk_amd import _lib, hazard, windfield  # noqa: E402

R_OUT = 500.0
DT = 3600.0
THR = np.arange(10, 81, 5).astype(np.float64)


def make_storms(rng, n_years, per_year):
    lon, lat, _, groups = make_tracks(rng, n_years, per_year)
    n, n_t = lon.shape
    v = np.clip(35 + np.cumsum(rng.normal(0.0, 1.0, (n, n_t)), axis=1), 15, 75)
    env = [rng.normal(0, 8, (n, n_t)) for _ in range(4)]
    tail = np.isnan(lon)
    v[tail] = np.nan
    for e in env:
        e[tail] = np.nan
    return lon, lat, v, env, groups


def run_gpu(L, h, dt, groups, slon, slat, substeps, K=3):
    dev = dt[0].device
    n_trk, n_t = dt[0].shape
    n_groups = int(groups.max()) + 1
    group_off = np.zeros(n_groups + 1, np.int64)
    group_off[1:] = np.cumsum(np.bincount(groups, minlength=n_groups))
    order = hazard._spatial_order(torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev), torch)
    sl, sa = torch.as_tensor(slon, device=dev)[order].contiguous(), torch.as_tensor(slat, device=dev)[order].contiguous()
    counts = torch.empty((len(slon), n_groups, THR.size), dtype=torch.int32, device=dev)
    trk = _lib.WindTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=dt[0].data_ptr(), lat=dt[1].data_ptr(), v=dt[2].data_ptr(),
                          u250=dt[3].data_ptr(), v250=dt[4].data_ptr(), u850=dt[5].data_ptr(), v850=dt[6].data_ptr(), rmax_km=None,
                          n_group=n_groups, group_off=group_off.ctypes.data_as(C.POINTER(C.c_int64)))
    prm = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=R_OUT, rmax_const_km=0.0, substeps=substeps)
    st = torch.cuda.current_stream(dev)

    def launch():
        if L.tcr_windfield_dev(h, C.byref(trk), C.byref(prm), len(slon), sl.data_ptr(), sa.data_ptr(), THR.size,
                               THR.ctypes.data_as(_lib.DP), counts.data_ptr(), None, C.c_void_p(st.cuda_stream)) != 0:
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
    if L.tcr_windfield_pairs(h, C.byref(pairs)) != 0:
        raise _lib.TcrError(L.tcr_last_error(h).decode())
    out = torch.empty_like(counts)
    out[order] = counts
    return float(np.median(ms)), ms, int(pairs.value), out.cpu().numpy()


def numpy_check(recs, dt, groups, slon, slat, substeps, idx):
    """The restatement on the sites `idx` and the storms of `recs` (dt: their planes): time per site on one core, and the GPU's
    site_max and counts against it."""
    n_groups = int(groups.max()) + 1
    t0 = time.perf_counter()
    lo, amb_any, amb_vals = WN.site_max(recs, slon[idx], slat[idx], R_OUT, 1.0)
    per_site = (time.perf_counter() - t0) / len(idx)
    r = windfield.site_wind(dt[0], dt[1], dt[2], dt[3:7], groups, torch.as_tensor(slon[idx], device=dt[0].device),
                            torch.as_tensor(slat[idx], device=dt[0].device), DT, r_out_km=R_OUT, substeps=substeps,
                            thresholds=THR, return_max=True)
    gm = r['site_max'].cpu().numpy()
    assert WN.allowed(gm, lo, amb_vals).all(), 'site_max differs from the restatement'
    und = WN.undecided(lo, amb_any, THR)
    assert np.array_equal(WN.counts(np.where(und, np.nan, gm), groups, n_groups, THR),
                          WN.counts(np.where(und, np.nan, lo), groups, n_groups, THR)), 'counts differ'
    assert np.array_equal(r['counts'].cpu().numpy(), WN.counts(gm, groups, n_groups, THR)), 'counts differ from site_max'
    return per_site, int(und.sum())


def main():
    quick = '--quick' in sys.argv
    rng = np.random.default_rng(7)
    n_years, per_year = (5, 200) if quick else (45, 1000)
    lon, lat, v, env, groups = make_storms(rng, n_years, per_year)
    n = WN.track_length(lon, lat, v, env)
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    L = _lib.lib()
    h = C.c_void_p()
    if L.tcr_ctx_create(0, C.byref(h)) != 0:
        raise _lib.TcrError(L.tcr_last_error(None).decode())
    sites = (('coast', coast_sites(rng, 1000 if quick else 10000)), ('grid', grid_sites()))
    results = []
    try:
        for substeps in (1, 4):
            records = int(np.where(n >= 2, (n - 1) * substeps + 1, 0).sum())
            # the restatement on a tenth of the storms, scaled to all of them
            sub = np.arange(0, lon.shape[0], 10)
            recs = WN.samples(lon[sub], lat[sub], v[sub], [e[sub] for e in env], DT, substeps=substeps)
            for name, (slon, slat) in sites:
                ms, all_ms, pairs, counts = run_gpu(L, h, dt, groups, slon, slat, substeps)
                raw = len(slon) * records
                idx = np.sort(np.random.default_rng(1).choice(len(slon), 3, replace=False))
                hit = np.nonzero(counts.sum(axis=(1, 2)))[0]
                if len(hit):
                    idx = np.unique(np.concatenate([idx, hit[np.linspace(0, len(hit) - 1, 3).astype(int)]]))
                per_site, undecided = numpy_check(recs, [x[sub] for x in dt], groups[sub], slon, slat, substeps, idx)
                np_total_s = per_site * len(slon) * (lon.shape[0] / len(sub))
                row = dict(workload=name, substeps=substeps, sites=len(slon), tracks=lon.shape[0], samples=lon.shape[1],
                           records=records, r_out_km=R_OUT, gpu_ms=round(ms, 3), gpu_ms_runs=[round(x, 3) for x in all_ms],
                           raw_pairs=raw, evaluated_pairs=pairs, culled_fraction=round(1 - pairs / raw, 5),
                           evaluated_pairs_per_s=pairs / (ms / 1e3), numpy_sites_checked=len(idx), numpy_storms_checked=len(sub),
                           numpy_undecided_pairs=undecided, numpy_extrapolated_s=round(np_total_s, 1),
                           speedup=round(np_total_s / (ms / 1e3), 1), sites_with_counts=int((counts.sum(axis=(1, 2)) > 0).sum()),
                           check='gpu == restatement (tolerance) on the checked sites x storms')
                results.append(row)
                print(json.dumps(row), flush=True)
    finally:
        L.tcr_ctx_destroy(h)
    for r in results:
        print('%-5s substeps %d, %6d sites: %9.2f ms, evaluated %.3g pairs/s (%.2f %% of %.3g pairs culled); restatement '
              '%.0f s extrapolated, speed-up %.0fx' % (r['workload'], r['substeps'], r['sites'], r['gpu_ms'], r['evaluated_pairs_per_s'],
                                                      100 * r['culled_fraction'], r['raw_pairs'], r['numpy_extrapolated_s'],
                                                      r['speedup']))


if __name__ == '__main__':
    main()
