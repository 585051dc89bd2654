"""Cost of the closest approach (csrc/tcr_approach.hip) next to the site hazard on the same shapes: tools/bench_windfield.py's
tracks (bench_common; 45 000 tracks x 361 samples; lon, lat and the gap-free v as vmax, so that both analyses have the same
records) and the 0.25-degree NA grid (87 001 sites), bands 50 / 100 / 200 km and the 15 default thresholds.

The hazard runs at the radius of the largest band on its own sphere (200 km x 6378 / 6378.1: the same angle), so at substeps 1 the
two scans evaluate the same (site, record) pairs (asserted).  Every variant is warmed up once, then the variants take turns for K
rounds (--rounds), each round in a random order of its own, each run between device events; reported are the runs and their medians in ms per call:

  (a) the full shape, planes off: tcr_hazard_dev (counts only), tcr_approach_dev at substeps 1 and at 4, tcr_approach_dev with the
      largest band alone (16 histogram cells per lane, the hazard's own, instead of 48: what the LDS of a wave costs), and with
      --parent-lib tcr_hazard_dev of a library built from the parent commit (that code path must not have moved);
  (b) a block of sites (every STRIDE-th tile of 64 sites in spatial order), planes on: tcr_hazard_dev with site_max,
      tcr_approach_dev with no plane and with all seven, at substeps 1 and 4.  The seven planes of the full shape are
      7 x 87 001 x 45 000 x 8 bytes = 219 GB, which no caller holds at once: planes are taken block by block (levels.device_levels).

and approach_over_hazard for each, the 4-substep figures over the 1-substep ones, the evaluated pairs and ns per evaluated pair.
The design expectation: with planes off the scan costs about what the hazard scan costs, since the loop adds one compare and two
selects to its fmax.

    python tools/bench_approach.py [--parent-lib PATH/libtcrisk_hip.so] [--quick] [--rounds K] [--out profiles/approach_bench.txt]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_common as BC
from bench_common import ROOT
import torch  # noqa: E402  (importing it does not touch the GPU)
from tropical_cyclone_risk_amd import _lib, approach  # noqa: E402

SEED = 7
DT = 3600.0
BANDS = np.array([50.0, 100.0, 200.0])
RE_KM = 6378.1
HAZARD_RE_KM = 6378.0
STRIDE = 10
K = 8


def alternating(fns, stream, k=K):
    """{name: runs in ms} of the launchers fns: one warm-up each, then k rounds in which they take turns, each between device events.
    Every round takes them in a seeded random order of its own, so that no variant always follows the same one."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    runs = {name: [] for name in fns}
    order = np.random.default_rng(SEED)
    for _ in range(k):
        for name in order.permutation(list(fns)):
            fn = fns[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream)
            torch.cuda.synchronize()
            runs[name].append(e0.elapsed_time(e1))
    return runs


def med(x):
    return round(float(np.median(x)), 3)


def main():
    args = sys.argv[1:]
    quick = '--quick' in args
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'approach_bench.txt')
    k = int(args[args.index('--rounds') + 1]) if '--rounds' in args else K
    lines = []

    def emit(**row):
        text = json.dumps(row)
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(SEED)
    n_years, per_year, _ = BC.sizes(quick)
    lon, lat, v, _, groups = BC.make_storms(rng, n_years, per_year)
    slon, slat = BC.grid_sites()
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in (lon, lat, v)]
    trk = BC.hazard_tracks(dt, groups)
    n_trk, n_groups = int(lon.shape[0]), int(trk.n_group)
    tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
    order = BC.sitescan.spatial_order(tl, ta, torch)
    sl, sa = tl[order].contiguous(), ta[order].contiguous()
    tiles = torch.arange(0, sl.shape[0], 64 * STRIDE, device=dev)
    pick = (tiles[:, None] + torch.arange(64, device=dev)[None, :]).reshape(-1)
    pick = pick[pick < sl.shape[0]]
    bl, ba = sl[pick].contiguous(), sa[pick].contiguous()
    thr = BC.THR
    st = torch.cuda.current_stream(dev)
    radius_h = float(BANDS[-1]) * HAZARD_RE_KM / RE_KM

    def hazard_call(lib, hh, x, y, counts, site_max):
        def launch():
            BC.check(lib, hh, lib.tcr_hazard_dev(hh, C.byref(trk), int(x.shape[0]), x.data_ptr(), y.data_ptr(), radius_h, thr.size,
                                                 thr.ctypes.data_as(_lib.DP), counts.data_ptr(),
                                                 None if site_max is None else site_max.data_ptr(), C.c_void_p(st.cuda_stream)))
        return launch

    def approach_call(lib, hh, x, y, substeps, counts, planes, bands=BANDS):
        prm = _lib.ApproachParams(dt_s=DT, substeps=substeps, rmax_const_km=0.0)
        arr = None
        if planes is not None:
            arr = (C.c_void_p * len(approach.PLANES))(*[p.data_ptr() for p in planes])

        def launch():
            BC.check(lib, hh, lib.tcr_approach_dev(hh, C.byref(trk), None, C.byref(prm), int(x.shape[0]), x.data_ptr(), y.data_ptr(),
                                                   bands.size, bands.ctypes.data_as(_lib.DP), thr.size, thr.ctypes.data_as(_lib.DP),
                                                   counts.data_ptr(), arr, C.c_void_p(st.cuda_stream)))
        launch.keep = (prm, arr)
        return launch

    def pairs_of(lib, hh, entry):
        n = C.c_int64()
        BC.check(lib, hh, getattr(lib, entry + '_pairs')(hh, C.byref(n)))
        return int(n.value)

    with BC.open_context() as (L, h):
        # (a) the full shape, planes off
        n_site = int(sl.shape[0])
        hc = torch.empty((n_site, n_groups, thr.size), dtype=torch.int32, device=dev)
        ac = {s: torch.empty((n_site, n_groups, BANDS.size, thr.size), dtype=torch.int32, device=dev) for s in (1, 4)}
        ac1 = torch.empty((n_site, n_groups, 1, thr.size), dtype=torch.int32, device=dev)
        fns = dict(hazard=hazard_call(L, h, sl, sa, hc, None), approach_sub1=approach_call(L, h, sl, sa, 1, ac[1], None),
                   approach_sub4=approach_call(L, h, sl, sa, 4, ac[4], None),
                   approach_one_band=approach_call(L, h, sl, sa, 1, ac1, None, BANDS[-1:].copy()))
        V = hv = None
        if '--parent-lib' in args:
            V = C.CDLL(os.path.abspath(args[args.index('--parent-lib') + 1]))
            V.tcr_last_error.restype = C.c_char_p
            V.tcr_last_error.argtypes = [C.c_void_p]
            V.tcr_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
            V.tcr_ctx_destroy.argtypes = [C.c_void_p]
            V.tcr_hazard_dev.argtypes = L.tcr_hazard_dev.argtypes
            assert not hasattr(V, 'tcr_approach_host'), 'the parent library already has the closest approach'
            hv = C.c_void_p()
            BC.check(V, None, V.tcr_ctx_create(0, C.byref(hv)))
            pc = torch.empty_like(hc)
            fns['hazard_parent'] = hazard_call(V, hv, sl, sa, pc, None)
        runs = alternating(fns, st, k)
        fns['approach_sub1']()                          # (the pair counter is the last call's)
        torch.cuda.synchronize()
        a_pairs, h_pairs = pairs_of(L, h, 'tcr_approach'), pairs_of(L, h, 'tcr_hazard')
        fns['approach_sub4']()
        torch.cuda.synchronize()
        a4_pairs = pairs_of(L, h, 'tcr_approach')
        # the largest band's counts are the hazard's where the closest record is also the strongest: never more
        checks = dict(largest_band_counts_at_most_hazard_counts=bool((ac[1][:, :, -1] <= hc).all()) and int(ac[1].sum()) > 0,
                      same_evaluated_pairs=a_pairs == h_pairs)
        row = dict(what='(a) full shape, planes off', sites=n_site, tracks=n_trk, samples=int(lon.shape[1]), bands_km=BANDS.tolist(),
                   n_bin=int(thr.size), hazard_radius_km=round(radius_h, 6), rounds=k,
                   hazard_ms=med(runs['hazard']), hazard_ms_runs=[round(x, 3) for x in runs['hazard']],
                   approach_ms=med(runs['approach_sub1']), approach_ms_runs=[round(x, 3) for x in runs['approach_sub1']],
                   approach_sub4_ms=med(runs['approach_sub4']), approach_sub4_ms_runs=[round(x, 3) for x in runs['approach_sub4']],
                   approach_over_hazard=round(med(runs['approach_sub1']) / med(runs['hazard']), 3),
                   approach_one_band_ms=med(runs['approach_one_band']),
                   approach_one_band_ms_runs=[round(x, 3) for x in runs['approach_one_band']],
                   approach_one_band_over_hazard=round(med(runs['approach_one_band']) / med(runs['hazard']), 3),
                   one_band_counts_equal_largest_band=bool(torch.equal(ac1[:, :, 0], ac[1][:, :, -1])),
                   approach_sub4_over_sub1=round(med(runs['approach_sub4']) / med(runs['approach_sub1']), 3),
                   evaluated_pairs=a_pairs, hazard_evaluated_pairs=h_pairs, sub4_evaluated_pairs=a4_pairs,
                   approach_ns_per_pair=round(med(runs['approach_sub1']) * 1e6 / max(a_pairs, 1), 5),
                   hazard_ns_per_pair=round(med(runs['hazard']) * 1e6 / max(h_pairs, 1), 5),
                   approach_sub4_ns_per_pair=round(med(runs['approach_sub4']) * 1e6 / max(a4_pairs, 1), 5),
                   passages_within_largest_band=int(ac[1][:, :, -1, 0].sum()), **checks)
        if V is not None:
            row.update(hazard_parent_ms=med(runs['hazard_parent']), hazard_parent_ms_runs=[round(x, 3) for x in runs['hazard_parent']],
                       hazard_over_parent=round(med(runs['hazard']) / med(runs['hazard_parent']), 3),
                       hazard_counts_equal_parent=bool(torch.equal(hc, pc)))
            V.tcr_ctx_destroy(hv)
        emit(**row)
        del hc, ac, ac1, fns

        # (b) a block of sites, planes on
        n_blk = int(bl.shape[0])
        hc = torch.empty((n_blk, n_groups, thr.size), dtype=torch.int32, device=dev)
        smax = torch.empty((n_blk, n_trk), dtype=torch.float64, device=dev)
        acb = torch.empty((n_blk, n_groups, BANDS.size, thr.size), dtype=torch.int32, device=dev)
        planes = [torch.empty((n_blk, n_trk), dtype=torch.float64, device=dev) for _ in approach.PLANES]
        fns = dict(hazard=hazard_call(L, h, bl, ba, hc, None), hazard_max=hazard_call(L, h, bl, ba, hc, smax))
        for s in (1, 4):
            fns['approach_sub%d' % s] = approach_call(L, h, bl, ba, s, acb, None)
            fns['approach_sub%d_planes' % s] = approach_call(L, h, bl, ba, s, acb, planes)
        runs = alternating(fns, st, k)
        fns['approach_sub1_planes']()
        torch.cuda.synchronize()
        vc, m = planes[2], smax
        both = ~torch.isnan(vc) & ~torch.isnan(m)
        checks.update(v_cpa_at_most_site_max=bool((vc[both] <= m[both]).all()),
                      cells_with_another_nan_than_the_hazard=int((torch.isnan(vc) != torch.isnan(m)).sum()))
        r = {k: med(x) for k, x in runs.items()}
        emit(what='(b) a block of sites (every %d-th tile of 64), planes on' % STRIDE, sites=n_blk, tracks=n_trk,
             plane_bytes=n_blk * n_trk * 8, rounds=k, ms=r, ms_runs={k: [round(y, 3) for y in x] for k, x in runs.items()},
             approach_over_hazard_planes_off=round(r['approach_sub1'] / r['hazard'], 3),
             approach_over_hazard_seven_planes=round(r['approach_sub1_planes'] / r['hazard'], 3),
             approach_seven_planes_over_hazard_with_site_max=round(r['approach_sub1_planes'] / r['hazard_max'], 3),
             sub4_over_sub1_planes_off=round(r['approach_sub4'] / r['approach_sub1'], 3),
             sub4_over_sub1_seven_planes=round(r['approach_sub4_planes'] / r['approach_sub1_planes'], 3),
             included_cells=int(both.sum()), v_cpa_at_most_site_max=checks['v_cpa_at_most_site_max'],
             cells_with_another_nan_than_the_hazard=checks['cells_with_another_nan_than_the_hazard'])
    if not quick:
        if os.path.exists(out_fn):                     # notes written next to the numbers are kept
            lines += [t.rstrip('\n') for t in open(out_fn) if t.startswith('#')]
        with open(out_fn, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    assert checks['largest_band_counts_at_most_hazard_counts'] and checks['same_evaluated_pairs'] and checks['v_cpa_at_most_site_max'], checks


if __name__ == '__main__':
    main()
