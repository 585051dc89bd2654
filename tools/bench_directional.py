"""Cost of the directional wind (csrc/tcr_directional.hip) next to the wind footprint on the same shapes, on tools/bench_windfield.py's
tracks (bench_common; 45 000 tracks x 361 samples, r_out = 500 km) and the 0.25-degree NA grid (87 001 sites), at substeps 1 and 4.

Reports, in ms per call (device events; every call is warmed up once, then the calls are timed in turn, K rounds, so that a
drift of the machine falls on all alike; every run and the medians):

  directional8  tcr_directional_dev with 8 sectors at 0 degrees and 7 thresholds (64 cells), counts only, no planes;
  directional4  the same with 4 sectors (32 cells);
  directional8_32cells  8 sectors with the first 3 thresholds: 32 cells, the 4-sector call's LDS with the 8-sector kernel;
  windfield     tcr_windfield_dev with the same 7 thresholds on the same inputs (that code path is the parent commit's);

and directional_over_footprint for each, the evaluated pairs (tcr_*_pairs: they must be equal) and ns per evaluated pair.  A wave's
histogram is 256 bytes of LDS per cell, n_sector (n_bin + 1) cells: 16 KB at 64 cells, which leaves a CU's 160 KB 10 waves where the
registers allow 20 (profiles/directional_resources.txt); the third call separates that from the kernel's instructions.  The counts
are checked against each other: the storms counted in some sector at a threshold are at least the footprint's (its peak is one of
the sectors'), and at most n_sector times as many.

    python tools/bench_directional.py [--quick] [--out profiles/directional_bench.txt]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_common as BC
from bench_common import ROOT
import torch  # noqa: E402  (importing it does not touch the GPU)
from tropical_cyclone_risk_amd import _lib, directional  # noqa: E402

SEED = 7
R_OUT = 500.0
DT = 3600.0
K = 5


def timed_in_turn(fns, stream, rounds=K):
    """[runs in ms] per function: one warm-up each, then `rounds` rounds of one timed call each, in turn."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    runs = [[] for _ in fns]
    for _ in range(rounds):
        for fn, out in zip(fns, runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
    return runs


def main():
    args = sys.argv[1:]
    quick = '--quick' in args
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'directional_bench.txt')
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(SEED)
    n_years, per_year, _ = BC.sizes(quick)
    lon, lat, v, env, groups = BC.make_storms(rng, n_years, per_year)
    slon, slat = BC.grid_sites()
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    trk = BC.wind_tracks(dt, groups)
    tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
    order = BC.sitescan.spatial_order(tl, ta, torch)
    sl, sa = tl[order].contiguous(), ta[order].contiguous()
    thr = np.ascontiguousarray(directional.DEFAULT_THRESHOLDS)
    n_site, n_bin, thr_p = len(slon), thr.size, thr.ctypes.data_as(_lib.DP)
    st = torch.cuda.current_stream(dev)
    stream = C.c_void_p(st.cuda_stream)
    c8 = torch.empty((n_site, trk.n_group, 8, n_bin), dtype=torch.int32, device=dev)
    c4 = torch.empty((n_site, trk.n_group, 4, n_bin), dtype=torch.int32, device=dev)
    c83 = torch.empty((n_site, trk.n_group, 8, 3), dtype=torch.int32, device=dev)
    cw = torch.empty((n_site, trk.n_group, n_bin), dtype=torch.int32, device=dev)
    with BC.open_context() as (L, h):
        for substeps in (1, 4):
            prm = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=R_OUT, rmax_const_km=0.0, substeps=substeps)

            def dir_call(n_sector, counts, n_thr=n_bin):
                return lambda: BC.check(L, h, L.tcr_directional_dev(h, C.byref(trk), C.byref(prm), n_site, sl.data_ptr(), sa.data_ptr(),
                                                                    n_sector, 0.0, n_thr, thr_p, counts.data_ptr(), None, stream))

            def wind_call():
                BC.check(L, h, L.tcr_windfield_dev(h, C.byref(trk), C.byref(prm), n_site, sl.data_ptr(), sa.data_ptr(), n_bin, thr_p,
                                                   cw.data_ptr(), None, stream))
            r8, rw, r4, r83 = timed_in_turn([dir_call(8, c8), wind_call, dir_call(4, c4), dir_call(8, c83, 3)], st)
            pairs = {}
            for name, fn, entry in (('directional8', dir_call(8, c8), 'tcr_directional'), ('directional4', dir_call(4, c4), 'tcr_directional'),
                                    ('windfield', wind_call, 'tcr_windfield')):
                fn()
                p = C.c_int64()
                BC.check(L, h, getattr(L, entry + '_pairs')(h, C.byref(p)))
                pairs[name] = int(p.value)
            n8, n4, nw = (x.sum(dim=1).cpu().numpy().astype(np.int64) for x in (c8, c4, cw))
            consistent = bool((n8.sum(axis=1) >= nw).all() and (n8.sum(axis=1) <= 8 * nw).all() and
                              (n4.sum(axis=1) >= nw).all() and (n4.sum(axis=1) <= 4 * nw).all() and
                              torch.equal(c83, c8[:, :, :, :3]))
            m8, m4, mw, m83 = float(np.median(r8)), float(np.median(r4)), float(np.median(rw)), float(np.median(r83))
            row = dict(what='tcr_directional_dev', workload='grid', substeps=substeps, sites=n_site, tracks=lon.shape[0],
                       samples=lon.shape[1], r_out_km=R_OUT, n_bin=n_bin, thresholds=[float(x) for x in thr], rounds=K,
                       directional8_ms=round(m8, 3), directional8_ms_runs=[round(x, 3) for x in r8],
                       directional4_ms=round(m4, 3), directional4_ms_runs=[round(x, 3) for x in r4],
                       directional8_32cells_ms=round(m83, 3), directional8_32cells_ms_runs=[round(x, 3) for x in r83],
                       windfield_ms=round(mw, 3), windfield_ms_runs=[round(x, 3) for x in rw],
                       directional_over_footprint=round(m8 / mw, 3), directional4_over_footprint=round(m4 / mw, 3),
                       directional8_32cells_over_footprint=round(m83 / mw, 3),
                       lds_bytes_per_wave=dict(directional8=256 * 8 * (n_bin + 1), directional4=256 * 4 * (n_bin + 1),
                                               directional8_32cells=256 * 8 * 4, windfield=256 * (n_bin + 1)),
                       evaluated_pairs=pairs['directional8'], evaluated_pairs_4=pairs['directional4'],
                       windfield_evaluated_pairs=pairs['windfield'],
                       directional8_ns_per_pair=round(m8 * 1e6 / max(pairs['directional8'], 1), 5),
                       directional4_ns_per_pair=round(m4 * 1e6 / max(pairs['directional4'], 1), 5),
                       windfield_ns_per_pair=round(mw * 1e6 / max(pairs['windfield'], 1), 5),
                       counts8_sum=int(n8.sum()), counts4_sum=int(n4.sum()), windfield_counts_sum=int(nw.sum()),
                       counts_consistent=consistent)
            emit(json.dumps(row))
            assert consistent and pairs['directional8'] == pairs['directional4'] == pairs['windfield']
    if not quick:
        with open(out_fn, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
