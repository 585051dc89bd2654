"""Throughput of the track climatology (csrc/tcr_climatology.hip) on 45 000 tracks (45 years x 1 000) x 361 samples
(bench_common.make_tracks), device tensors in and out:

  na_box   the 0.25-degree NA box (lon 260..350, lat 0..60: 360 x 240 cells), thresholds 33 and 50 m/s, one group per year
  globe    the 1-degree globe (360 x 180 cells), the CLI's default thresholds (Saffir-Simpson 1-5), summed over groups

Reports ms per call (device events, median of 3 after a warm-up; the call zeroes its maps), live samples/s and the (storm, cell)
pairs counted; the NumPy restatement (tests/climatology_numpy.py) on one core on a tenth of the storms, extrapolated to all of
them.  The GPU's per-storm outputs on that tenth, and its maps of that tenth run on its own, equal the restatement with `==`.

    python tools/bench_climatology.py [--quick]
"""
import ctypes as C
import json
import sys
import time

import numpy as np

import bench_common as BC
from bench_common import timed
import torch  # noqa: E402
from tests import climatology_numpy as CN  # noqa: E402
from tropical_cyclone_risk_amd import _lib, climatology  # noqa: E402


def _check(got, want, keys):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)
        assert a.shape == b.shape and np.array_equal(a, b), k


def main():
    quick = '--quick' in sys.argv
    rng = np.random.default_rng(7)
    n_years, per_year, _ = BC.sizes(quick)
    lon, lat, vmax, years = BC.make_tracks(rng, n_years, per_year)
    n_trk, n_t = lon.shape
    live = int((~np.isnan(lon) & ~np.isnan(lat)).sum())
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in (lon, lat, vmax)]
    st = torch.cuda.current_stream(dev)
    sub = np.arange(0, n_trk, 10)
    workloads = (('na_box', climatology.CellGrid.from_bounds(260, 350, 0, 60, 0.25), np.array([33.0, 50.0]), years, n_years),
                 ('globe', climatology.CellGrid.from_bounds(0, 360, -90, 90, 1), np.array(climatology.SAFFIR_SIMPSON),
                  np.zeros(n_trk, np.int64), 1))
    with BC.open_context() as (L, h):
        trk = BC.hazard_tracks(dt)
        for name, grid, thr, groups, n_groups in workloads:
            shape = (n_groups, grid.nlat, grid.nlon)
            i32 = dict(dtype=torch.int32, device=dev)
            res = dict(track=torch.empty(shape, **i32), exceed=torch.empty((n_groups, thr.size) + shape[1:], **i32),
                       genesis=torch.empty(shape, **i32), lmi=torch.empty(shape, **i32),
                       pdi=torch.empty(shape, dtype=torch.int64, device=dev), genesis_k=torch.empty(n_trk, **i32),
                       lmi_v=torch.empty(n_trk, dtype=torch.float64, device=dev), lmi_k=torch.empty(n_trk, **i32),
                       pdi_storm=torch.empty(n_trk, dtype=torch.int64, device=dev))
            out = _lib.ClimOut(**{k: v.data_ptr() for k, v in res.items()})
            gi = torch.as_tensor(groups.astype(np.int32), device=dev)
            cg = grid._c()

            def run():
                BC.check(L, h, L.tcr_climatology_dev(h, C.byref(trk), gi.data_ptr(), n_groups, C.byref(cg), thr.size,
                                                     thr.ctypes.data_as(_lib.DP), C.byref(out), C.c_void_p(st.cuda_stream)))
            ms, runs = timed(run, st)
            got = {k: v.cpu().numpy() for k, v in res.items()}

            # the restatement on one core on a tenth of the storms; the GPU on the same tenth, and its per-storm outputs, equal it
            g_grid = (grid.lon0, grid.dlon, grid.nlon, grid.lat0, grid.dlat, grid.nlat)
            t0 = time.perf_counter()
            want = CN.climatology(lon[sub], lat[sub], vmax[sub], groups[sub], n_groups, g_grid, thr)
            np_s = (time.perf_counter() - t0) * n_trk / sub.size
            _check({k: got[k][sub] for k in climatology.STORM_FIELDS}, want, climatology.STORM_FIELDS)
            part = climatology.track_climatology(lon[sub], lat[sub], vmax[sub], groups[sub], grid, thr, n_groups=n_groups)
            _check(part, want, climatology.MAP_FIELDS + climatology.STORM_FIELDS)

            pairs = int(got['track'].sum())
            row = dict(workload=name, tracks=n_trk, samples=n_t, live_samples=live, cells=[grid.nlon, grid.nlat], groups=n_groups,
                       thresholds=thr.tolist(), gpu_ms=round(ms, 4), gpu_ms_runs=[round(x, 4) for x in runs],
                       live_samples_per_s=live / (ms / 1e3), storm_cell_pairs=pairs,
                       storms_with_genesis_in_grid=int(got['genesis'].sum()), storms_with_lmi_in_grid=int(got['lmi'].sum()),
                       numpy_tracks_checked=int(sub.size), numpy_extrapolated_s=round(np_s, 2), speedup=round(np_s / (ms / 1e3), 1),
                       check='gpu == restatement on the tenth (maps of the tenth run alone, per-storm outputs of the full run)')
            print(json.dumps(row), flush=True)
            print('%s: %d tracks x %d samples on %d x %d cells, %d groups: %.3f ms, %.3g live samples/s, %d storm-cell pairs; '
                  'NumPy restatement %.1f s extrapolated, speed-up %.0fx'
                  % (name, n_trk, n_t, grid.nlon, grid.nlat, n_groups, ms, row['live_samples_per_s'], pairs, np_s, row['speedup']),
                  flush=True)


if __name__ == '__main__':
    main()
