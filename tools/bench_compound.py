"""Cost of the compound wind-rain scan (csrc/tcr_compound.hip) next to the two single-hazard calls it replaces, on
tools/bench_windfield.py's site sets and tracks (bench_common; 45 000 tracks x 361 samples, both radii 500 km, c = 1, rm modelled):

  coast  10^4 coast-like sites          grid   the 0.25-degree NA grid (87 001 sites)

The rain reads (lon, lat, v) of bench_common.make_storms as (lon, lat, vmax), as tools/bench_rainfall.py does.  One process, one
context; at substeps 1 and 4, in ms per call (device events, every one of 3 runs after a warm-up, and their median):
tcr_compound_dev (stat = total, no value planes), tcr_windfield_dev and tcr_rainfall_dev on the same thresholds, the ratio
compound / (wind + rain), and the evaluated pairs of the three (tcr_*_pairs).  The compound's two marginals are checked against
the counts of the two calls (equal integers).

--bins NW,NR takes the first NW wind and NR rain thresholds (the scan's LDS histogram is 256 (NW + 1) (NR + 1) bytes per wave).

    python tools/bench_compound.py [--quick] [--bins NW,NR] [--out profiles/compound_bench.txt]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_common as BC
from bench_common import ROOT
import torch  # noqa: E402  (importing it does not touch the GPU)
from tropical_cyclone_risk_amd import _lib, rainfall  # noqa: E402

SEED = 7
R_OUT = 500.0
DT = 3600.0
WTHR = np.arange(20, 71, 10).astype(np.float64)            # 6 wind thresholds (m/s)
RTHR = np.arange(50, 401, 50).astype(np.float64)           # 8 rain thresholds (mm): 7 x 9 = 63 cells


def main():
    global WTHR, RTHR
    args = sys.argv[1:]
    quick = '--quick' in args
    if '--bins' in args:
        nw, nr = (int(x) for x in args[args.index('--bins') + 1].split(','))
        WTHR, RTHR = WTHR[:nw], RTHR[:nr]
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'compound_bench.txt')
    rng = np.random.default_rng(SEED)
    n_years, per_year, n_coast = BC.sizes(quick)
    lon, lat, v, env, groups = BC.make_storms(rng, n_years, per_year)
    sites = (('coast', BC.coast_sites(rng, n_coast)), ('grid', BC.grid_sites()))
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    wtrk, htrk = BC.wind_tracks(dt, groups), BC.hazard_tracks(dt[:3], groups)
    n_groups = wtrk.n_group
    st = torch.cuda.current_stream(dev)
    a, b = rainfall.DEFAULT_COEFFICIENTS
    lines = []
    with BC.open_context() as (L, h):
        for substeps in (1, 4):
            wprm = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=R_OUT, rmax_const_km=0.0, substeps=substeps)
            rprm = _lib.RainParams(dt_s=DT, r_out_km=R_OUT, v_lo_kt=35.0, v_hi_kt=155.0, a=(C.c_double * 4)(*a), b=(C.c_double * 4)(*b),
                                   substeps=substeps, stat=_lib.RAIN_TOTAL)
            for name, (slon, slat) in sites:
                n_site = len(slon)
                tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
                order = BC.sitescan.spatial_order(tl, ta, torch)
                sl, sa = tl[order].contiguous(), ta[order].contiguous()
                cc = torch.empty((n_site, n_groups, WTHR.size + 1, RTHR.size + 1), dtype=torch.int32, device=dev)
                cw = torch.empty((n_site, n_groups, WTHR.size), dtype=torch.int32, device=dev)
                cr = torch.empty((n_site, n_groups, RTHR.size), dtype=torch.int32, device=dev)
                wp, rp = WTHR.ctypes.data_as(_lib.DP), RTHR.ctypes.data_as(_lib.DP)
                stream = C.c_void_p(st.cuda_stream)
                calls = dict(
                    compound=lambda: BC.check(L, h, L.tcr_compound_dev(h, C.byref(wtrk), dt[2].data_ptr(), C.byref(wprm), C.byref(rprm), n_site,
                                                                       sl.data_ptr(), sa.data_ptr(), WTHR.size, wp, RTHR.size, rp,
                                                                       cc.data_ptr(), None, None, stream)),
                    windfield=lambda: BC.check(L, h, L.tcr_windfield_dev(h, C.byref(wtrk), C.byref(wprm), n_site, sl.data_ptr(), sa.data_ptr(),
                                                                         WTHR.size, wp, cw.data_ptr(), None, stream)),
                    rainfall=lambda: BC.check(L, h, L.tcr_rainfall_dev(h, C.byref(htrk), C.byref(rprm), n_site, sl.data_ptr(), sa.data_ptr(),
                                                                       RTHR.size, rp, cr.data_ptr(), None, stream)))
                row = dict(what='tcr_compound_dev total vs tcr_windfield_dev + tcr_rainfall_dev', workload=name, substeps=substeps,
                           sites=n_site, tracks=lon.shape[0], samples=lon.shape[1], r_out_km=R_OUT, n_wbin=int(WTHR.size),
                           n_rbin=int(RTHR.size))
                for what, fn in calls.items():
                    ms, runs = BC.timed(fn, st)
                    pairs = C.c_int64()
                    BC.check(L, h, getattr(L, 'tcr_%s_pairs' % what)(h, C.byref(pairs)))
                    row[what + '_ms'], row[what + '_ms_runs'], row[what + '_pairs'] = round(ms, 3), [round(x, 3) for x in runs], pairs.value
                row['compound_over_wind_plus_rain'] = round(row['compound_ms'] / (row['windfield_ms'] + row['rainfall_ms']), 3)
                assert torch.equal(cc[..., 1:, 0], cw) and torch.equal(cc[..., 0, 1:], cr), 'a marginal differs from its single-hazard call'
                row['joint_counts_sum'] = int(cc[..., 1:, 1:].sum())
                row['check'] = 'both marginals == the single-hazard counts'
                print(json.dumps(row), flush=True)
                lines.append(json.dumps(row))
    if not quick:
        with open(out_fn, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
