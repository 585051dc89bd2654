"""Throughput of the site-hazard kernels (csrc/tcr_hazard.hip) on two workloads, against NumPy on a subsample:

  coast  10^4 coast-like sites (bench_common.coast_sites) x 45 000 tracks (45 years x 1 000) x 361 samples
  grid   the 0.25-degree NA grid (bench_common.grid_sites: 87 001 sites) x the same tracks

Tracks are bench_common.make_tracks' seeded random walks.  Reports ms per call (device events, median of 3 after a warm-up), pairs/s counted two ways
(raw: sites x live samples; evaluated: the (site, sample) distance tests left after culling, tcr_hazard_pairs), and NumPy (the
notebook's haversine + where + nanmax, tests/hazard_numpy.py) on a few sites, extrapolated to the same raw work.  The GPU result
on those sites is checked against NumPy.

    python tools/bench_hazard.py [--quick]
"""
import json
import sys
import time

import numpy as np

import bench_common as BC
from bench_common import R_KM, THR, coast_sites, grid_sites, make_tracks
import torch  # noqa: E402
from tests import hazard_numpy as HN  # noqa: E402
from tropical_cyclone_risk_amd import hazard  # noqa: E402


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
    n_years, per_year, n_coast = BC.sizes(quick)
    lon, lat, vmax, groups = make_tracks(rng, n_years, per_year)
    live = int((~np.isnan(lon)).sum())
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in (lon, lat, vmax)]
    trk = BC.hazard_tracks(dt, groups)
    results = []
    with BC.open_context() as (L, h):
        for name, (slon, slat) in (('coast', coast_sites(rng, n_coast)), ('grid', grid_sites())):
            ms, all_ms, pairs, counts = BC.time_site_scan(L, h, 'tcr_hazard', trk, (), (R_KM,), slon, slat)
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
    for r in results:
        print('%-5s %6d sites: %9.2f ms  raw %.3g pairs/s, evaluated %.3g pairs/s (%.2f %% culled); NumPy %.3g pairs/s '
              '-> %.0f s extrapolated, speed-up %.0fx' % (r['workload'], r['sites'], r['gpu_ms'], r['raw_pairs_per_s'],
                                                       r['evaluated_pairs_per_s'], 100 * r['culled_fraction'],
                                                       r['numpy_pairs_per_s'], r['numpy_extrapolated_s'], r['speedup']))


if __name__ == '__main__':
    main()
