"""Cost of the rainfall footprint (csrc/tcr_rainfall.hip) next to the wind footprint on the same shapes, on
tools/bench_windfield.py's site sets and tracks (bench_common; 45 000 tracks x 361 samples, r_out = 500 km):

  coast  10^4 coast-like sites          grid   the 0.25-degree NA grid (87 001 sites)

The rain reads (lon, lat, v) of bench_common.make_storms as (lon, lat, vmax).  Reports, in ms per call (device events, every one
of 3 runs after a warm-up, and their median):

  (a) with --parent-lib: tcr_hazard_dev (100 km), tcr_windfield_dev and tcr_loss_dev (substeps 1) of a library built from the
      parent commit and of this tree's library, each in a process of its own on the same box, the two alternating for two rounds:
      the scan's existing instantiations must cost what they did (per round: this tree's median <= the parent's slowest of its
      three runs + the parent's spread; pairs, counts and losses equal);
  (b) tcr_rainfall_dev, stat = total, at substeps 1 and 4, and tcr_windfield_dev on the same shape in the same session: ms,
      evaluated pairs (tcr_*_pairs), ns per evaluated pair of both, and their ratio.  The GPU result is checked against the
      restatement (tests/rainfall_numpy.py) on a few sites x a tenth of the storms.

    python tools/bench_rainfall.py [--parent-lib PATH/libtcrisk_hip.so] [--quick] [--out profiles/rainfall_bench.txt]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

import bench_common as BC
from bench_common import ROOT, THR
import torch  # noqa: E402  (importing it does not touch the GPU)
from tests import rainfall_numpy as RN  # noqa: E402
from tropical_cyclone_risk_amd import _lib, rainfall  # noqa: E402

SEED = 7
R_OUT = 500.0
DT = 3600.0


def workload(quick):
    rng = np.random.default_rng(SEED)
    n_years, per_year, n_coast = BC.sizes(quick)
    lon, lat, v, env, groups = BC.make_storms(rng, n_years, per_year)
    sites = (('coast', BC.coast_sites(rng, n_coast)), ('grid', BC.grid_sites()))
    return lon, lat, v, env, groups, sites


def rain_params(substeps, stat=_lib.RAIN_TOTAL):
    a, b = rainfall.DEFAULT_COEFFICIENTS
    return _lib.RainParams(dt_s=DT, r_out_km=R_OUT, v_lo_kt=35.0, v_hi_kt=155.0, a=(C.c_double * 4)(*a), b=(C.c_double * 4)(*b),
                           substeps=substeps, stat=stat)


def wind_params(substeps):
    return _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=R_OUT, rmax_const_km=0.0, substeps=substeps)


def existing_only(lib_path, quick):
    """Child process: the three existing scans of the library at lib_path on both site sets; one JSON line."""
    _lib._pin_hip_runtime()
    L = C.CDLL(lib_path)
    L.tcr_last_error.restype = C.c_char_p
    L.tcr_last_error.argtypes = [C.c_void_p]
    L.tcr_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.tcr_ctx_destroy.argtypes = [C.c_void_p]
    L.tcr_hazard_dev.argtypes = [C.c_void_p, C.POINTER(_lib.HazardTracks), C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_int32,
                                 _lib.DP, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tcr_hazard_pairs.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.tcr_windfield_dev.argtypes = [C.c_void_p, C.POINTER(_lib.WindTracks), C.POINTER(_lib.WindParams), C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_int32, _lib.DP, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tcr_windfield_pairs.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.tcr_loss_dev.argtypes = [C.c_void_p, C.POINTER(_lib.WindTracks), C.POINTER(_lib.WindParams), C.POINTER(_lib.LossParams),
                               C.c_int64] + [C.c_void_p] * 4 + [C.c_int32, _lib.DP] + [C.c_void_p] * 6
    lon, lat, v, env, groups, sites = workload(quick)
    n_groups = int(groups.max()) + 1
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    st = torch.cuda.current_stream(dev)
    wtrk, htrk = BC.wind_tracks(dt, groups), BC.hazard_tracks(dt[:3], groups)
    wprm = wind_params(1)
    lprm = _lib.LossParams(v_thresh=25.7, v_half=74.7)
    out = {}
    with BC.open_context(L) as (L, h):
        for name, (slon, slat) in sites:
            row = {}
            for what, trk, before, after in (('hazard', htrk, (), (BC.R_KM,)), ('windfield', wtrk, (C.byref(wprm),), ())):
                ms, runs, pairs, counts = BC.time_site_scan(L, h, 'tcr_' + what, trk, before, after, slon, slat)
                row[what] = dict(ms=round(ms, 3), runs=[round(x, 3) for x in runs], pairs=pairs, counts_sum=int(counts.sum()))
            n_site = len(slon)
            tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
            order = BC.sitescan.spatial_order(tl, ta, torch)
            sl, sa = tl[order].contiguous(), ta[order].contiguous()
            sv = torch.as_tensor(np.random.default_rng(SEED + 1).lognormal(13.0, 1.5, n_site), device=dev)[order].contiguous()
            counts = torch.empty((n_site, n_groups, THR.size), dtype=torch.int32, device=dev)
            ev, agg, mx, sl_ = (torch.empty(n, dtype=torch.float64, device=dev) for n in (lon.shape[0], n_groups, n_groups, n_site))

            def loss_call():
                BC.check(L, h, L.tcr_loss_dev(h, C.byref(wtrk), C.byref(wprm), C.byref(lprm), n_site, sl.data_ptr(), sa.data_ptr(),
                                              sv.data_ptr(), None, THR.size, THR.ctypes.data_as(_lib.DP), counts.data_ptr(), ev.data_ptr(),
                                              agg.data_ptr(), mx.data_ptr(), sl_.data_ptr(), C.c_void_p(st.cuda_stream)))
            ms, runs = BC.timed(loss_call, st)
            row['loss'] = dict(ms=round(ms, 3), runs=[round(x, 3) for x in runs], events_with_loss=int((ev > 0).sum()),
                               counts_sum=int(counts.sum()), aal=float(agg.sum()) / n_groups)
            out[name] = row
    print('RESULT ' + json.dumps(out), flush=True)


def child(lib_path, quick):
    cmd = [sys.executable, os.path.abspath(__file__), '--existing-only', lib_path] + (['--quick'] if quick else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit('run of %s failed (%d):\n%s' % (lib_path, p.returncode, p.stderr[-2000:]))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])


def numpy_check(lon, lat, v, dt, groups, slon, slat, substeps, idx):
    """The restatement on the sites `idx` and the storms given (dt: their planes on the device): seconds per site on one core;
    the GPU's site_total and counts are checked against it."""
    n_groups = int(groups.max()) + 1
    recs = RN.records(lon, lat, v, DT, substeps)
    t0 = time.perf_counter()
    want, n_band = RN.site_values(recs, slon[idx], slat[idx], R_OUT)
    per_site = (time.perf_counter() - t0) / len(idx)
    assert n_band == 0, 'a pair of the subsample is in the r_out band'
    r = rainfall.site_rain(dt[0], dt[1], dt[2], groups, torch.as_tensor(slon[idx], device=dt[0].device),
                           torch.as_tensor(slat[idx], device=dt[0].device), DT, r_out_km=R_OUT, substeps=substeps, thresholds=THR,
                           return_values=True)
    got = r['site_total'].cpu().numpy()
    assert RN.close(got, want).all(), 'site_total differs from the restatement'
    near = RN.near_threshold(want, THR)
    assert np.array_equal(RN.counts(np.where(near, np.nan, got), groups, n_groups, THR),
                          RN.counts(np.where(near, np.nan, want), groups, n_groups, THR)), 'counts differ'
    assert np.array_equal(r['counts'].cpu().numpy(), RN.counts(got, groups, n_groups, THR)), 'counts differ from site_total'
    return per_site, int((~np.isnan(want)).sum())


def main():
    args = sys.argv[1:]
    quick = '--quick' in args
    if '--existing-only' in args:
        return existing_only(args[args.index('--existing-only') + 1], quick)
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'rainfall_bench.txt')
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    # (a) one process per library, the two alternating (parent, this tree, parent, this tree), before this process touches the GPU:
    # a difference that follows the library shows in both rounds, one that follows the session does not
    if '--parent-lib' in args:
        parent_lib = os.path.abspath(args[args.index('--parent-lib') + 1])
        for rnd in (1, 2):
            a_parent, a_this = child(parent_lib, quick), child(_lib.LIB_PATH, quick)
            for name in ('coast', 'grid'):
                for what in ('hazard', 'windfield', 'loss'):
                    p, t = a_parent[name][what], a_this[name][what]
                    same = all(p[k] == t[k] for k in p if k not in ('ms', 'runs'))
                    spread = max(p['runs']) - min(p['runs'])
                    ok = t['ms'] <= max(p['runs']) + spread
                    emit(json.dumps(dict(what='(a) tcr_%s_dev' % what, workload=name, round=rnd, parent_ms_runs=p['runs'],
                                         this_ms_runs=t['runs'], parent_median=p['ms'], this_median=t['ms'], parent_slowest=max(p['runs']),
                                         parent_spread=round(spread, 3), same_results=same, condition_met=bool(ok and same))))

    # (b) rainfall and footprint on the same shapes, one session
    lon, lat, v, env, groups, sites = workload(quick)
    n = RN.track_length(lon, lat, v)
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    wtrk, htrk = BC.wind_tracks(dt, groups), BC.hazard_tracks(dt[:3], groups)
    sub = np.arange(0, lon.shape[0], 10)                    # the restatement's tenth of the storms
    with BC.open_context() as (L, h):
        for substeps in (1, 4):
            records = int(np.where(n >= 2, (n - 1) * substeps + 1, 0).sum())
            rprm, wprm = rain_params(substeps), wind_params(substeps)
            for name, (slon, slat) in sites:
                w_ms, w_runs, w_pairs, _ = BC.time_site_scan(L, h, 'tcr_windfield', wtrk, (C.byref(wprm),), (), slon, slat)
                ms, runs, pairs, counts = BC.time_site_scan(L, h, 'tcr_rainfall', htrk, (C.byref(rprm),), (), slon, slat)
                idx = np.sort(np.random.default_rng(1).choice(len(slon), 3, replace=False))
                hit = np.nonzero(counts.sum(axis=(1, 2)))[0]
                if len(hit):
                    idx = np.unique(np.concatenate([idx, hit[np.linspace(0, len(hit) - 1, 3).astype(int)]]))
                per_site, n_values = numpy_check(lon[sub], lat[sub], v[sub], [x[sub] for x in dt], groups[sub], slon, slat, substeps, idx)
                np_total_s = per_site * len(slon) * (lon.shape[0] / len(sub))
                emit(json.dumps(dict(
                    what='(b) tcr_rainfall_dev total', workload=name, substeps=substeps, sites=len(slon), tracks=lon.shape[0],
                    samples=lon.shape[1], records=records, r_out_km=R_OUT, rain_ms=round(ms, 3), rain_ms_runs=[round(x, 3) for x in runs],
                    windfield_ms=round(w_ms, 3), windfield_ms_runs=[round(x, 3) for x in w_runs], rain_over_windfield=round(ms / w_ms, 3),
                    raw_pairs=len(slon) * records, rain_evaluated_pairs=pairs, windfield_evaluated_pairs=w_pairs,
                    culled_fraction=round(1 - pairs / (len(slon) * records), 5), rain_ns_per_pair=round(ms * 1e6 / pairs, 5),
                    windfield_ns_per_pair=round(w_ms * 1e6 / w_pairs, 5), numpy_sites_checked=len(idx), numpy_storms_checked=len(sub),
                    numpy_values_checked=n_values, numpy_extrapolated_s=round(np_total_s, 1), speedup=round(np_total_s / (ms / 1e3), 1),
                    sites_with_counts=int((counts.sum(axis=(1, 2)) > 0).sum()),
                    check='gpu == restatement (tolerance) on the checked sites x storms')))
    if not quick:
        with open(out_fn, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
