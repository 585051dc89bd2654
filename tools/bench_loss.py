"""Cost of the portfolio loss (csrc/tcr_loss.hip) next to the wind footprint it is fused into, on tools/bench_windfield.py's
site sets and tracks (bench_common; 45 000 tracks x 361 samples, r_out = 500 km, substeps 1, c = 1, rm modelled):

  coast  10^4 coast-like sites          grid   the 0.25-degree NA grid (87 001 sites)

Exposure values are seeded lognormal (median exp(13), sigma 1.5).  Reports, in ms per call (device events, every one of 3 runs
after a warm-up, and their median):

  (a) tcr_windfield_dev of a library built from the parent commit (--parent-lib) and of this tree's library, each in a process
      of its own on the same box: the footprint's existing instantiations must cost what they did;
  (b) tcr_loss_dev (sites already in spatial order, as (a)), and loss.portfolio_loss on a context that persists (with the site
      and storm permutations of the Python front end, as (c));
  (c) the unfused route on `coast`, where its 3.6 GB matrix fits: windfield.site_wind(return_max=True) on a context that
      persists, then the damage function and the sums in torch.  Its event losses are checked against (b)'s.

    python tools/bench_loss.py --parent-lib PATH/libtcrisk_hip.so [--quick] [--out profiles/loss_bench.txt]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np

import bench_common as BC
from bench_common import ROOT
import torch  # noqa: E402  (importing it does not touch the GPU)
from tropical_cyclone_risk_amd import _lib, loss, sitescan, windfield  # noqa: E402

SEED = 7
THR = BC.THR


def workload(quick):
    rng = np.random.default_rng(SEED)
    n_years, per_year, n_coast = BC.sizes(quick)
    lon, lat, v, env, groups = BC.make_storms(rng, n_years, per_year)
    sites = (('coast', BC.coast_sites(rng, n_coast)), ('grid', BC.grid_sites()))
    return lon, lat, v, env, groups, sites


def windfield_only(lib_path, quick):
    """Child process: tcr_windfield_dev of the library at lib_path on both site sets; one JSON line."""
    _lib._pin_hip_runtime()
    L = C.CDLL(lib_path)
    L.tcr_last_error.restype = C.c_char_p
    L.tcr_last_error.argtypes = [C.c_void_p]
    L.tcr_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.tcr_ctx_destroy.argtypes = [C.c_void_p]
    L.tcr_windfield_dev.argtypes = [C.c_void_p, C.POINTER(_lib.WindTracks), C.POINTER(_lib.WindParams), C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_int32, _lib.DP, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tcr_windfield_pairs.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lon, lat, v, env, groups, sites = workload(quick)
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    trk = BC.wind_tracks(dt, groups)
    prm = _lib.WindParams(dt_s=3600.0, ck_cd=1.0, r_out_km=500.0, rmax_const_km=0.0, substeps=1)
    out = {}
    with BC.open_context(L) as (L, h):
        for name, (slon, slat) in sites:
            ms, runs, pairs, counts = BC.time_site_scan(L, h, 'tcr_windfield', trk, (C.byref(prm),), (), slon, slat)
            out[name] = dict(ms=round(ms, 3), runs=[round(x, 3) for x in runs], pairs=pairs, counts_sum=int(counts.sum()))
    print('RESULT ' + json.dumps(out), flush=True)


def child(lib_path, quick):
    cmd = [sys.executable, os.path.abspath(__file__), '--windfield-only', lib_path] + (['--quick'] if quick else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit('windfield run of %s failed (%d):\n%s' % (lib_path, p.returncode, p.stderr[-2000:]))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])


def main():
    args = sys.argv[1:]
    quick = '--quick' in args
    if '--windfield-only' in args:
        return windfield_only(args[args.index('--windfield-only') + 1], quick)
    if '--parent-lib' not in args:
        raise SystemExit(__doc__)
    parent_lib = os.path.abspath(args[args.index('--parent-lib') + 1])
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'loss_bench.txt')
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    # (a) one process per library, one after the other, before this process touches the GPU
    a_parent, a_this = child(parent_lib, quick), child(_lib.LIB_PATH, quick)
    for name in ('coast', 'grid'):
        p, t = a_parent[name], a_this[name]
        same = p['pairs'] == t['pairs'] and p['counts_sum'] == t['counts_sum']
        spread = max(p['runs']) - min(p['runs'])
        ok = t['ms'] <= max(p['runs']) + spread
        emit(json.dumps(dict(what='(a) tcr_windfield_dev', workload=name, parent_ms_runs=p['runs'], this_ms_runs=t['runs'],
                             parent_median=p['ms'], this_median=t['ms'], parent_slowest=max(p['runs']), parent_spread=round(spread, 3),
                             same_pairs_and_counts=same, condition_1_met=bool(ok and same))))

    lon, lat, v, env, groups, sites = workload(quick)
    n_groups = int(groups.max()) + 1
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    st = torch.cuda.current_stream(dev)
    trk = BC.wind_tracks(dt, groups)
    n_trk = lon.shape[0]
    keep = {}                           # the last result of a timed function

    def ms_runs(fn):
        return [round(x, 3) for x in BC.timed(fn, st)[1]]
    with BC.open_context() as (L, h):
        eng = types.SimpleNamespace(h=h)
        for name, (slon, slat) in sites:
            n_site = len(slon)
            value = np.random.default_rng(SEED + 1).lognormal(13.0, 1.5, n_site)
            tl, ta, tv = (torch.as_tensor(x, device=dev) for x in (slon, slat, value))
            # (b) the entry point itself, sites in spatial order
            order = sitescan.spatial_order(tl, ta, torch)
            sl, sa, sv = tl[order].contiguous(), ta[order].contiguous(), tv[order].contiguous()
            wprm = _lib.WindParams(dt_s=3600.0, ck_cd=1.0, r_out_km=500.0, rmax_const_km=0.0, substeps=1)
            lprm = _lib.LossParams(v_thresh=loss.V_THRESH, v_half=loss.V_HALF)
            counts = torch.empty((n_site, n_groups, THR.size), dtype=torch.int32, device=dev)
            ev, agg, mx, sl_ = (torch.empty(n, dtype=torch.float64, device=dev) for n in (n_trk, n_groups, n_groups, n_site))

            def direct():
                BC.check(L, h, L.tcr_loss_dev(h, C.byref(trk), C.byref(wprm), C.byref(lprm), n_site, sl.data_ptr(), sa.data_ptr(),
                                              sv.data_ptr(), None, THR.size, THR.ctypes.data_as(_lib.DP), counts.data_ptr(), ev.data_ptr(),
                                              agg.data_ptr(), mx.data_ptr(), sl_.data_ptr(), C.c_void_p(st.cuda_stream)))
            b_ms = ms_runs(direct)
            kw = dict(r_out_km=500.0, substeps=1, ck_cd=1.0, thresholds=THR, engine=eng, n_groups=n_groups)
            api_ms = ms_runs(lambda: keep.update(res=loss.portfolio_loss(dt[0], dt[1], dt[2], dt[3:7], groups, tl, ta, tv, 3600.0, **kw)))
            res = keep['res']
            assert torch.equal(res['event_loss'], ev) and torch.equal(res['year_agg'], agg) and torch.equal(res['year_max'], mx)
            row = dict(what='(b) tcr_loss_dev', workload=name, sites=n_site, tracks=n_trk, loss_ms_runs=b_ms,
                       loss_median=float(np.median(b_ms)), portfolio_loss_api_ms_runs=api_ms, api_median=float(np.median(api_ms)),
                       windfield_this_median=a_this[name]['ms'], loss_over_windfield=round(float(np.median(b_ms)) / a_this[name]['ms'], 3),
                       aal=float(agg.sum()) / n_groups, events_with_loss=int((ev > 0).sum()))
            emit(json.dumps(row))
            if name != 'coast':
                continue
            # (c) the unfused route: the footprint matrix, then the damage function and the sums in torch
            g = torch.as_tensor(groups, device=dev)

            def unfused():
                w = windfield.site_wind(dt[0], dt[1], dt[2], dt[3:7], groups, tl, ta, 3600.0, return_max=True, **kw)
                x = (torch.nan_to_num(w['site_max'], nan=0.0) - loss.V_THRESH).clamp_(min=0.0).div_(loss.V_HALF - loss.V_THRESH)
                x3 = x * x * x
                T = x3.div_(1.0 + x3).mul_(tv[:, None])
                e = T.sum(dim=0)
                keep['un'] = dict(event_loss=e, site_loss=T.sum(dim=1), counts=w['counts'],
                                  year_agg=torch.zeros(n_groups, dtype=torch.float64, device=dev).index_add_(0, g, e),
                                  year_max=torch.zeros(n_groups, dtype=torch.float64, device=dev).index_reduce_(0, g, e, 'amax'))
            c_ms = ms_runs(unfused)
            un = keep.pop('un')
            err = float(((un['event_loss'] - res['event_loss']).abs() / res['event_loss'].clamp(min=1e-300)).max())
            assert err <= (n_site + 16) * 2.0 ** -52 and torch.equal(un['counts'], res['counts']), err
            emit(json.dumps(dict(what='(c) site_wind(return_max) + torch', workload=name, unfused_ms_runs=c_ms,
                                 unfused_median=float(np.median(c_ms)), site_max_gb=round(n_site * n_trk * 8 / 1e9, 2),
                                 event_loss_max_rel_diff=err, fused_api_over_unfused=round(float(np.median(api_ms) / np.median(c_ms)), 3),
                                 condition_2_met=bool(np.median(b_ms) <= np.median(c_ms)))))
            del un
            torch.cuda.empty_cache()
    if not quick:
        with open(out_fn, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
