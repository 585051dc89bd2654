"""Throughput of landfall detection (csrc/tcr_landfall.hip) on the reference's 0.125-degree land mask (tests/golden/ref_land.nc):

  detect  45 000 tracks (45 years x 1 000) x 361 samples (bench_common.make_tracks), device tensors in and out, no flags
  coast   the 10 000-site coast landfall hazard (bench_common.coast_sites, R = 100 km) on the device event planes

Reports ms per call (device events, median of 3 after a warm-up) and live samples/s, and the NumPy restatement
(tests/landfall_numpy.py) on one core on a subsample of the tracks, extrapolated to all of them; the GPU events of that subsample
are checked against it bit for bit.

    python tools/bench_landfall.py [--quick]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

import bench_common as BC
from bench_common import timed
import torch  # noqa: E402
from tests import landfall_numpy as LN  # noqa: E402
from tropical_cyclone_risk_amd import _lib, landfall  # noqa: E402

CAP = 16


def main():
    quick = '--quick' in sys.argv
    rng = np.random.default_rng(7)
    n_years, per_year, n_coast = BC.sizes(quick)
    lon, lat, vmax, groups = BC.make_tracks(rng, n_years, per_year)
    n_trk, n_t = lon.shape
    live = int((~np.isnan(lon) & ~np.isnan(lat)).sum())
    grid = landfall.read_land(os.path.join(BC.ROOT, 'tests', 'golden', 'ref_land.nc'))
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in (lon, lat, vmax)]
    st = torch.cuda.current_stream(dev)
    with BC.open_context() as (L, h):
        g = _lib.LandGrid(nlon=grid.lon.size, nlat=grid.lat.size, lon=grid.lon.ctypes.data, lat=grid.lat.ctypes.data,
                          land=grid.land.ctypes.data)
        BC.check(L, h, L.tcr_land_upload(h, C.byref(g)))
        trk = BC.hazard_tracks(dt)
        n_lf = torch.empty(n_trk, dtype=torch.int32, device=dev)
        ev_k = torch.empty((n_trk, CAP), dtype=torch.int32, device=dev)
        planes = [torch.empty((n_trk, CAP), dtype=torch.float64, device=dev) for _ in range(4)]

        def detect():
            BC.check(L, h, L.tcr_landfall_dev(h, C.byref(trk), CAP, n_lf.data_ptr(), ev_k.data_ptr(), *[p.data_ptr() for p in planes],
                                              None, C.c_void_p(st.cuda_stream)))
        ms, runs = timed(detect, st)
        n = n_lf.cpu().numpy()
        assert n.max() <= CAP, n.max()

    # the restatement on one core, on a subsample; the GPU's events there must equal it bit for bit
    sub = np.arange(0, n_trk, 10)
    t0 = time.perf_counter()
    want = LN.landfalls(lon[sub], lat[sub], vmax[sub], grid.lon, grid.lat, grid.land)
    np_s = (time.perf_counter() - t0) * n_trk / sub.size
    m = want['k'].shape[1]
    assert np.array_equal(n[sub], want['n_landfall'])
    assert np.array_equal(ev_k.cpu().numpy()[sub, :m], want['k'])
    for p, key in zip(planes, landfall.EVENT_FIELDS):
        assert np.array_equal(p.cpu().numpy()[sub, :m].view(np.int64), want[key].view(np.int64)), key

    row = dict(workload='detect', tracks=n_trk, samples=n_t, live_samples=live, land_grid=list(grid.land.shape), gpu_ms=round(ms, 4),
               gpu_ms_runs=[round(x, 4) for x in runs], live_samples_per_s=live / (ms / 1e3),
               track_bytes=2 * n_trk * n_t * 8, storms_with_landfall=int((n > 0).sum()), landfalls=int(n.sum()),
               max_landfalls=int(n.max()), numpy_tracks_checked=int(sub.size), numpy_extrapolated_s=round(np_s, 2),
               speedup=round(np_s / (ms / 1e3), 1), check='gpu == restatement on the subsample, bit for bit')
    print(json.dumps(row), flush=True)

    # coast landfall hazard on the device events
    ev = dict(k=ev_k, lon=planes[0], lat=planes[1], v_landfall=planes[2], v_inland=planes[3], n_landfall=n_lf)
    slon, slat = BC.coast_sites(rng, n_coast)
    ts = [torch.as_tensor(a, device=dev) for a in (slon, slat)]
    out = {}

    def site():
        out['r'] = landfall.landfall_site_hazard(ev, groups, ts[0], ts[1], radius_km=BC.R_KM, thresholds=BC.THR)
    t0 = time.perf_counter()
    sms, sruns = timed(site, st)
    counts = out['r']['counts'].cpu().numpy()
    row2 = dict(workload='coast_landfall_hazard', sites=len(slon), tracks=n_trk, event_columns=CAP, gpu_ms=round(sms, 3),
                gpu_ms_runs=[round(x, 3) for x in sruns], sites_with_counts=int((counts.sum(axis=(1, 2)) > 0).sum()),
                note='landfall_site_hazard end to end (ordering, hazard kernels) on [n_trk][%d] event planes' % CAP)
    print(json.dumps(row2), flush=True)
    print('detect %d tracks x %d samples: %.3f ms, %.3g live samples/s; NumPy restatement %.1f s extrapolated, speed-up %.0fx; '
          '%d storms make %d landfalls' % (n_trk, n_t, ms, row['live_samples_per_s'], np_s, row['speedup'], row['storms_with_landfall'],
                                           row['landfalls']))
    print('coast landfall hazard, %d sites: %.3f ms' % (len(slon), sms))


if __name__ == '__main__':
    main()
