"""Throughput of the wind-footprint kernels (csrc/tcr_windfield.hip) on two site sets, against the NumPy restatement on a subsample:

  coast  10^4 coast-like sites (bench_common.coast_sites) x 45 000 tracks (45 years x 1 000) x 361 samples
  grid   the 0.25-degree NA grid (bench_common.grid_sites: 87 001 sites) x the same tracks

Tracks are bench_common.make_storms' seeded random walks.  r_out = 500 km, substeps 1 and 4, c = 1, rm modelled.  Reports ms per call (device events, median of 3
after a warm-up), the raw pairs (sites x samples and sub-samples), the evaluated pairs left after culling (tcr_windfield_pairs)
and the culled fraction, evaluated pairs/s, and the restatement (tests/windfield_numpy.py) on a few sites on one core,
extrapolated to all sites; the GPU result on those sites is checked against it.

    python tools/bench_windfield.py [--quick]
"""
import ctypes as C
import json
import sys
import time

import numpy as np

import bench_common as BC
from bench_common import THR
import torch  # noqa: E402
from tests import windfield_numpy as WN  # noqa: E402
from tropical_cyclone_risk_amd import _lib, windfield  # noqa: E402

R_OUT = 500.0
DT = 3600.0


def run_gpu(L, h, trk, slon, slat, substeps):
    """bench_common.time_site_scan of tcr_windfield (r_out = 500 km, c = 1, rm modelled)."""
    prm = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=R_OUT, rmax_const_km=0.0, substeps=substeps)
    return BC.time_site_scan(L, h, 'tcr_windfield', trk, (C.byref(prm),), (), slon, slat)


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
    n_years, per_year, n_coast = BC.sizes(quick)
    lon, lat, v, env, groups = BC.make_storms(rng, n_years, per_year)
    n = WN.track_length(lon, lat, v, env)
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    trk = BC.wind_tracks(dt, groups)
    sites = (('coast', BC.coast_sites(rng, n_coast)), ('grid', BC.grid_sites()))
    results = []
    with BC.open_context() as (L, h):
        for substeps in (1, 4):
            records = int(np.where(n >= 2, (n - 1) * substeps + 1, 0).sum())
            # the restatement on a tenth of the storms, scaled to all of them
            sub = np.arange(0, lon.shape[0], 10)
            recs = WN.samples(lon[sub], lat[sub], v[sub], [e[sub] for e in env], DT, substeps=substeps)
            for name, (slon, slat) in sites:
                ms, all_ms, pairs, counts = run_gpu(L, h, trk, slon, slat, substeps)
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
    for r in results:
        print('%-5s substeps %d, %6d sites: %9.2f ms, evaluated %.3g pairs/s (%.2f %% of %.3g pairs culled); restatement '
              '%.0f s extrapolated, speed-up %.0fx' % (r['workload'], r['substeps'], r['sites'], r['gpu_ms'], r['evaluated_pairs_per_s'],
                                                      100 * r['culled_fraction'], r['raw_pairs'], r['numpy_extrapolated_s'],
                                                      r['speedup']))


if __name__ == '__main__':
    main()
