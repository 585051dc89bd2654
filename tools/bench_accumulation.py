"""Cost of the rain accumulation windows (csrc/tcr_accumulation.hip) next to the rainfall footprint's storm total on the same
input: bench_common's tracks (45 000 tracks x 361 samples, r_out = 500 km) on the 0.25-degree NA grid (87 001 sites), at substeps
1 and 4, for the windows 6/12/24 h and 6/24/72 h.  The ring of running depths costs LDS (512 bytes per sample of the longest
window and wave), so the open question is how the cost depends on the longest window.  Reports, in ms per call (device events,
every one of 3 runs after a warm-up, and their median), one JSON line per case:

  (a) with --parent-lib: tcr_rainfall_dev, stat = total, of a library built from the parent commit and of this tree's library,
      each in a process of its own on the same box, the two alternating for two rounds.  Only the two spare slots of the records
      k_rain_prep writes changed, so the call must cost what it did (per round: this tree's median <= the parent's slowest of its
      three runs + the parent's spread; pairs and counts equal);
  (b) tcr_accumulation_dev (no planes) and tcr_rainfall_dev total in one session: ms, evaluated pairs of both (equal), ns per
      pair, accumulation_over_total, and multi_equals_singles: on every 40th site x every 10th storm (a plane of the whole
      workload is 31 GB) each window alone gives the bits it has in the joint call.  The GPU result is checked against the
      restatement (tests/accumulation_numpy.py) on a few sites x a tenth of the storms.

    python tools/bench_accumulation.py [--parent-lib PATH/libtcrisk_hip.so] [--quick] [--out profiles/accumulation_bench.txt]
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

import bench_common as BC
from bench_common import ROOT, THR
import torch  # noqa: E402  (importing it does not touch the GPU)
from bench_rainfall import DT, R_OUT, SEED, rain_params  # noqa: E402
from tests import accumulation_numpy as AN  # noqa: E402
from tests import rainfall_numpy as RN  # noqa: E402
from tropical_cyclone_risk_amd import _lib, accumulation  # noqa: E402

WINDOW_SETS = ((6, 12, 24), (6, 24, 72))
SUBSTEPS = (1, 4)


def workload(quick):
    rng = np.random.default_rng(SEED)
    n_years, per_year, _ = BC.sizes(quick)
    lon, lat, v, _, groups = BC.make_storms(rng, n_years, per_year)
    return lon, lat, v, groups, BC.grid_sites()


def total_only(lib_path, quick):
    """Child process: tcr_rainfall_dev total of the library at lib_path on the grid, at both substeps; one JSON line."""
    _lib._pin_hip_runtime()
    L = C.CDLL(lib_path)
    L.tcr_last_error.restype = C.c_char_p
    L.tcr_last_error.argtypes = [C.c_void_p]
    L.tcr_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.tcr_ctx_destroy.argtypes = [C.c_void_p]
    L.tcr_rainfall_dev.argtypes = [C.c_void_p, C.POINTER(_lib.HazardTracks), C.POINTER(_lib.RainParams), C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_int32, _lib.DP, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tcr_rainfall_pairs.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lon, lat, v, groups, (slon, slat) = workload(quick)
    dev = torch.device('cuda', 0)
    htrk = BC.hazard_tracks([torch.as_tensor(a, device=dev) for a in (lon, lat, v)], groups)
    out = {}
    with BC.open_context(L) as (L, h):
        for sub in SUBSTEPS:
            prm = rain_params(sub)
            ms, runs, pairs, counts = BC.time_site_scan(L, h, 'tcr_rainfall', htrk, (C.byref(prm),), (), slon, slat)
            out[str(sub)] = dict(ms=round(ms, 3), runs=[round(x, 3) for x in runs], pairs=pairs, counts_sum=int(counts.sum()))
    print('RESULT ' + json.dumps(out), flush=True)


def child(lib_path, quick):
    cmd = [sys.executable, os.path.abspath(__file__), '--total-only', lib_path] + (['--quick'] if quick else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit('run of %s failed (%d):\n%s' % (lib_path, p.returncode, p.stderr[-2000:]))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])


def time_accumulation(L, h, trk, prm, m, slon, slat):
    """tcr_accumulation_dev without planes, sites in spatial order: (median ms, runs, evaluated pairs, sum of the counts)."""
    dev = trk.keep[0][0].device
    tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
    order = BC.sitescan.spatial_order(tl, ta, torch)
    sl, sa = tl[order].contiguous(), ta[order].contiguous()
    counts = torch.empty((len(slon), trk.n_group, len(m), THR.size), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)
    mm = np.asarray(m, np.int32)

    def launch():
        BC.check(L, h, L.tcr_accumulation_dev(h, C.byref(trk), C.byref(prm), len(slon), sl.data_ptr(), sa.data_ptr(), len(m),
                                              mm.ctypes.data_as(C.POINTER(C.c_int32)), THR.size, THR.ctypes.data_as(_lib.DP),
                                              counts.data_ptr(), None, C.c_void_p(st.cuda_stream)))
    ms, runs = BC.timed(launch, st)
    pairs = C.c_int64()
    BC.check(L, h, L.tcr_accumulation_pairs(h, C.byref(pairs)))
    return ms, runs, int(pairs.value), int(counts.sum())


def subset_checks(lon, lat, v, dt, groups, slon, slat, sub, windows):
    """On every 40th site x every 10th storm: each window alone gives the bits it has in the joint call; and on a few of those
    sites the joint call is the restatement's (tolerance).  (multi_equals_singles, values checked)"""
    n_groups = int(groups.max()) + 1
    dev = dt[0].device
    sl, sa = torch.as_tensor(slon[::40], device=dev), torch.as_tensor(slat[::40], device=dev)
    kw = dict(thresholds=THR, r_out_km=R_OUT, substeps=sub, n_groups=n_groups, return_values=True)
    joint = accumulation.site_accumulation(dt[0], dt[1], dt[2], groups, sl, sa, DT, windows_h=windows, **kw)
    same = True
    for i, w in enumerate(windows):
        one = accumulation.site_accumulation(dt[0], dt[1], dt[2], groups, sl, sa, DT, windows_h=[w], **kw)
        same = same and torch.equal(one['site_window'][0].view(torch.int64), joint['site_window'][i].view(torch.int64)) \
            and torch.equal(one['counts'][:, :, 0], joint['counts'][:, :, i])
    hit = np.nonzero(joint['counts'].sum(dim=(1, 2, 3)).cpu().numpy())[0]
    idx = np.unique(hit[np.linspace(0, len(hit) - 1, 4).astype(int)]) if len(hit) else np.arange(3)
    want, n_band = AN.site_windows(RN.records(lon, lat, v, DT, sub), slon[::40][idx], slat[::40][idx], R_OUT, DT, sub, windows)
    assert n_band == 0, 'a pair of the subsample is in the r_out band'
    got = joint['site_window'][:, torch.as_tensor(idx, device=dev)].cpu().numpy()
    assert RN.close(got, want).all(), 'site_window differs from the restatement'
    return bool(same), int((~np.isnan(want)).sum())


def main():
    args = sys.argv[1:]
    quick = '--quick' in args
    if '--total-only' in args:
        return total_only(args[args.index('--total-only') + 1], quick)
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'accumulation_bench.txt')
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    # (a) one process per library, the two alternating, before this process touches the GPU
    parent = {}
    if '--parent-lib' in args:
        parent_lib = os.path.abspath(args[args.index('--parent-lib') + 1])
        for rnd in (1, 2):
            a_parent, a_this = child(parent_lib, quick), child(_lib.LIB_PATH, quick)
            parent = a_parent
            for sub in SUBSTEPS:
                p, t = a_parent[str(sub)], a_this[str(sub)]
                same = p['pairs'] == t['pairs'] and p['counts_sum'] == t['counts_sum']
                spread = max(p['runs']) - min(p['runs'])
                ok = t['ms'] <= max(p['runs']) + spread
                emit(json.dumps(dict(what='(a) tcr_rainfall_dev total', workload='grid', substeps=sub, round=rnd, parent_ms_runs=p['runs'],
                                     this_ms_runs=t['runs'], parent_median=p['ms'], this_median=t['ms'], parent_slowest=max(p['runs']),
                                     parent_spread=round(spread, 3), same_results=same, condition_met=bool(ok and same))))

    # (b) the windows and the total on the same input, one session
    lon, lat, v, groups, (slon, slat) = workload(quick)
    n = RN.track_length(lon, lat, v)
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in (lon, lat, v)]
    htrk = BC.hazard_tracks(dt, groups)
    tenth = np.arange(0, lon.shape[0], 10)
    with BC.open_context() as (L, h):
        for sub in SUBSTEPS:
            records = int(np.where(n >= 2, (n - 1) * sub + 1, 0).sum())
            prm = rain_params(sub)
            t_ms, t_runs, t_pairs, _ = BC.time_site_scan(L, h, 'tcr_rainfall', htrk, (C.byref(prm),), (), slon, slat)
            for windows in WINDOW_SETS:
                ms, runs, pairs, csum = time_accumulation(L, h, htrk, prm, windows, slon, slat)
                same, n_values = subset_checks(lon[tenth], lat[tenth], v[tenth], [x[tenth] for x in dt], groups[tenth], slon, slat, sub,
                                               list(windows))
                lds = 512 * (windows[-1] + 1) + 256 * len(windows) * (THR.size + 1)
                row = dict(what='(b) tcr_accumulation_dev', workload='grid', substeps=sub, windows_h=list(windows), sites=len(slon),
                           tracks=lon.shape[0], samples=lon.shape[1], records=records, r_out_km=R_OUT, n_bin=int(THR.size),
                           lds_bytes_per_wave=lds, accumulation_ms=round(ms, 3), accumulation_ms_runs=[round(x, 3) for x in runs],
                           total_ms=round(t_ms, 3), total_ms_runs=[round(x, 3) for x in t_runs],
                           accumulation_over_total=round(ms / t_ms, 3), accumulation_evaluated_pairs=pairs, total_evaluated_pairs=t_pairs,
                           pairs_equal=pairs == t_pairs, accumulation_ns_per_pair=round(ms * 1e6 / pairs, 5),
                           total_ns_per_pair=round(t_ms * 1e6 / t_pairs, 5), counts_sum=csum, multi_equals_singles=same,
                           multi_equals_singles_on='every 40th site x every 10th storm', numpy_values_checked=n_values,
                           check='gpu == restatement (tolerance) on the checked sites x storms')
                if parent:
                    row.update(parent_total_ms=parent[str(sub)]['ms'], parent_total_ms_runs=parent[str(sub)]['runs'],
                               parent_total_evaluated_pairs=parent[str(sub)]['pairs'])
                emit(json.dumps(row))
    if not quick:
        with open(out_fn, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
