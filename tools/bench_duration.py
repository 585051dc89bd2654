"""Cost of the wind duration (csrc/tcr_duration.hip) next to the wind footprint on the same shapes, on tools/bench_windfield.py's
tracks (bench_common; 45 000 tracks x 361 samples, r_out = 500 km) and the 0.25-degree NA grid (87 001 sites), at substeps 1 and 4.

Reports, in ms per call (device events, every one of 3 runs after a warm-up, and their median):

  duration      tcr_duration_dev with the three default levels (34, 50, 64 kt) and the six default durations, counts and
                half_steps, no planes;
  windfield     one tcr_windfield_dev call on the same inputs in the same session (that code path is the parent commit's);
  singles       three tcr_duration_dev calls with one level each, and their sum;

and duration / windfield, duration / singles, the evaluated pairs (tcr_*_pairs: the same for both) and ns per evaluated pair.  The
expectation to confirm or refute: one multi-level call costs well under three footprint calls and little over one.  The counts and
totals of the multi-level call must equal those of the three single-level calls, and with --check (--quick sizes only) the planes
are compared with the restatement (tests/duration_numpy.py) on a few sites.

    python tools/bench_duration.py [--quick] [--check] [--out profiles/duration_bench.txt]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_common as BC
from bench_common import ROOT
import torch  # noqa: E402  (importing it does not touch the GPU)
from tropical_cyclone_risk_amd import _lib, duration  # noqa: E402

SEED = 7
R_OUT = 500.0
DT = 3600.0


def time_duration(L, h, trk, prm, levels, thr, sl, sa, K=3):
    """(median ms, runs, pairs, counts, half_steps) of tcr_duration_dev on sites already in spatial order."""
    dev = sl.device
    n_site, n_level, n_bin = int(sl.shape[0]), len(levels), len(thr)
    counts = torch.empty((n_site, trk.n_group, n_level, n_bin), dtype=torch.int32, device=dev)
    half = torch.empty((n_site, trk.n_group, n_level), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev)
    lev, th = np.ascontiguousarray(levels, dtype=np.float64), np.ascontiguousarray(thr, dtype=np.float64)

    def launch():
        BC.check(L, h, L.tcr_duration_dev(h, C.byref(trk), C.byref(prm), n_site, sl.data_ptr(), sa.data_ptr(), n_level,
                                          lev.ctypes.data_as(_lib.DP), n_bin, th.ctypes.data_as(_lib.DP), counts.data_ptr(),
                                          half.data_ptr(), None, C.c_void_p(st.cuda_stream)))
    ms, runs = BC.timed(launch, st, K)
    pairs = C.c_int64()
    BC.check(L, h, L.tcr_duration_pairs(h, C.byref(pairs)))
    return ms, runs, int(pairs.value), counts.cpu().numpy(), half.cpu().numpy()


def numpy_check(lon, lat, v, env, dt, groups, slon, slat, substeps, idx):
    """The restatement on the sites `idx` and the storms given (dt: their planes on the device): every cell within its bounds."""
    from tests import duration_numpy as DN
    from tests import windfield_numpy as WN
    recs = WN.samples(lon, lat, v, env, DT, substeps=substeps)
    lo, hi, _, inc_any, inc_sure = DN.duration(recs, slon[idx], slat[idx], R_OUT, 1.0, duration.DEFAULT_LEVELS)
    dev = dt[0].device
    r = duration.site_duration(dt[0], dt[1], dt[2], dt[3:7], groups, torch.as_tensor(slon[idx], device=dev),
                               torch.as_tensor(slat[idx], device=dev), DT, ck_cd=1.0, r_out_km=R_OUT, substeps=substeps,
                               return_hours=True)
    sh = r['site_hours'].cpu().numpy()
    nan = np.isnan(sh)
    H = np.rint(np.where(nan, 0.0, sh) / r['hours_per_half_step']).astype(np.int64)
    assert not (nan[0] & inc_sure).any() and not (~nan[0] & ~inc_any).any(), 'NaN differs from the restatement'
    assert (nan | ((lo <= H) & (H <= hi))).all(), 'site_hours outside the restatement\'s bounds'
    return int((~nan).sum())


def main():
    args = sys.argv[1:]
    quick = '--quick' in args
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'duration_bench.txt')
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
    wtrk = BC.wind_tracks(dt, groups)
    tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
    order = BC.sitescan.spatial_order(tl, ta, torch)
    sl, sa = tl[order].contiguous(), ta[order].contiguous()
    levels, thr = duration.DEFAULT_LEVELS, duration.DEFAULT_HOURS
    with BC.open_context() as (L, h):
        for substeps in (1, 4):
            prm = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=R_OUT, rmax_const_km=0.0, substeps=substeps)
            w_ms, w_runs, w_pairs, _ = BC.time_site_scan(L, h, 'tcr_windfield', wtrk, (C.byref(prm),), (), slon, slat)
            ms, runs, pairs, counts, half = time_duration(L, h, wtrk, prm, levels, thr, sl, sa)
            singles = [time_duration(L, h, wtrk, prm, levels[l:l + 1], thr, sl, sa) for l in range(len(levels))]
            same = all(np.array_equal(s[3][:, :, 0], counts[:, :, l]) and np.array_equal(s[4][:, :, 0], half[:, :, l])
                       for l, s in enumerate(singles))
            s_ms = sum(s[0] for s in singles)
            row = dict(what='tcr_duration_dev', workload='grid', substeps=substeps, sites=len(slon), tracks=lon.shape[0],
                       samples=lon.shape[1], r_out_km=R_OUT, levels=[round(float(x), 4) for x in levels], n_bin=len(thr),
                       duration_ms=round(ms, 3), duration_ms_runs=[round(x, 3) for x in runs],
                       windfield_ms=round(w_ms, 3), windfield_ms_runs=[round(x, 3) for x in w_runs],
                       single_level_ms=[round(s[0], 3) for s in singles], three_singles_ms=round(s_ms, 3),
                       duration_over_windfield=round(ms / w_ms, 3), duration_over_three_windfield=round(ms / (3 * w_ms), 3),
                       duration_over_three_singles=round(ms / s_ms, 3), evaluated_pairs=pairs, windfield_evaluated_pairs=w_pairs,
                       duration_ns_per_pair=round(ms * 1e6 / max(pairs, 1), 5), windfield_ns_per_pair=round(w_ms * 1e6 / max(w_pairs, 1), 5),
                       counts_sum=int(counts.sum()), half_steps_sum=int(half.sum()), multi_equals_singles=bool(same))
            if quick and '--check' in args:
                sub = np.arange(0, lon.shape[0], 10)
                hit = np.nonzero(counts.sum(axis=(1, 2, 3)))[0]
                idx = np.unique(order.cpu().numpy()[hit[np.linspace(0, len(hit) - 1, 4).astype(int)]]) if len(hit) else np.arange(3)
                row['restatement_cells_checked'] = numpy_check(lon[sub], lat[sub], v[sub], [e[sub] for e in env], [x[sub] for x in dt],
                                                               groups[sub], slon, slat, substeps, idx)
            emit(json.dumps(row))
            assert same and pairs == w_pairs
    if not quick:
        with open(out_fn, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
