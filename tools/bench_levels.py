"""Cost of return levels (levels.py, csrc/tcr_select.hip) on tools/bench_windfield.py's tracks and site sets (bench_common; 45 000
tracks x 361 samples, r_out = 500 km, substeps 1):

  coast  10^4 coast-like sites          grid   the 0.25-degree NA grid (87 001 sites)

Reports medians of 3 runs after a warm-up:

  (a) k_row_select alone (tcr_select_dev, device events) on one block of each site set, the block of the middle of the spatial
      order as levels.site_return_levels cuts it (max_bytes = 2^31) and the wind footprint fills it: ms, the plane's bytes over
      that time against 8 TB/s, and the share of rows with more than TCR_SELECT_LDS_KEYS values (the global path).  Next to it,
      tcr_windfield_dev on the same block with and without the plane (device events): the scan of the select's own block, and what
      writing the plane costs it;
  (b) the blocked levels.site_return_levels pass against the plain windfield.site_wind call without a plane on the same sites (host
      clock around work that ends in a device synchronise; one library context for all): the ratio, and the overhead split by
      running the same blocks three ways: site_wind per block without the plane (the blocking itself: per-block preparation and
      culling tables), with the plane (its write, and site_scan's copy back to the caller's order), and the driver (the select and
      the bookkeeping), and the driver again with max_bytes = 2^33 and 2^35 (fewer blocks; the result must be the same bits).  The
      blocked counts must equal the plain call's, and the levels of a few sites the restatement's (tests/levels_numpy.py) on the
      footprint's own rows;
  (c) with --variant-lib: tcr_select_dev on every block of both site sets, this tree's library against a library built from a copy
      of the tree with another TCR_SELECT_LDS_KEYS in the header (the constant has no build flag), the two alternating, 6 runs
      each: ms per block, totals, and the results compared bit for bit.

    python tools/bench_levels.py [--variant-lib PATH/libtcrisk_hip.so] [--quick] [--out profiles/return_levels_bench.txt]

With --tail K (K = 256 for the record) it measures the tail fit (levels.row_tail, csrc/tcr_tail.hip) instead, on the same tracks,
site sets and middle block, return periods 100, 250, 500 and 1000 years, and writes profiles/tail_levels_bench.txt:

  (d) k_row_tail alone (tcr_tail_dev, device events) against k_row_select alone on that plane, the select of this tree's library
      and, with --parent-lib, of a library built from the parent commit (the two selects must agree in bits and in time: the tail
      shares the select's routines and must not have changed its code), next to the scan of the block; the rows checked against the
      restatement (tests/tail_numpy.py): threshold, xi, sigma and n_valid in bits, and the largest
      |gpu - ref| / (|u| + |ref - u|) over their levels;
  (e) the blocked levels.site_return_levels pass at one block (max_bytes = 2^35) with and without tail_exceedances = K (host
      clock, each run ending in a device synchronise); the keys the two share must be the same bits.

    python tools/bench_levels.py --tail 256 [--parent-lib PATH/libtcrisk_hip.so] [--quick] [--out profiles/tail_levels_bench.txt]
"""
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np

import bench_common as BC
from bench_common import ROOT, THR
import torch  # noqa: E402  (importing it does not touch the GPU)
from tests import levels_numpy as LN  # noqa: E402
from tests import tail_numpy as TN  # noqa: E402
from tropical_cyclone_risk_amd import _lib, levels, sitescan, windfield  # noqa: E402

SEED = 7
R_OUT = 500.0
DT = 3600.0
MAX_BYTES = 2 ** 31
HBM_TBS = 8.0


def host_timed(fn, K=3):
    """(median, runs) in ms by the host clock, K runs after a warm-up, each ending in a device synchronise."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(K):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), ms


def main():
    args = sys.argv[1:]
    quick = '--quick' in args
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'return_levels_bench.txt')
    lines = []

    def emit(**row):
        text = json.dumps(row)
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(SEED)
    n_years, per_year, n_coast = BC.sizes(quick)
    lon, lat, v, env, groups = BC.make_storms(rng, n_years, per_year)
    sites = (('coast', BC.coast_sites(rng, n_coast)), ('grid', BC.grid_sites()))
    n_trk = lon.shape[0]
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    wtrk = BC.wind_tracks(dt, groups)
    wprm = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=R_OUT, rmax_const_km=0.0, substeps=1)
    T = levels.DEFAULT_RETURN_PERIODS
    k, _ = levels.ranks_of_periods(T, n_years)
    ranks = (C.c_int64 * k.size)(*k.tolist())
    st = torch.cuda.current_stream(dev)
    block = max(64, MAX_BYTES // (8 * n_trk)) // 64 * 64
    with BC.open_context() as (L, h):
        eng = types.SimpleNamespace(h=h)
        variant = None
        if '--variant-lib' in args:
            V = C.CDLL(os.path.abspath(args[args.index('--variant-lib') + 1]))
            V.tcr_last_error.restype = C.c_char_p
            V.tcr_last_error.argtypes = [C.c_void_p]
            V.tcr_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
            V.tcr_ctx_destroy.argtypes = [C.c_void_p]
            V.tcr_select_dev.argtypes = L.tcr_select_dev.argtypes
            hv = C.c_void_p()
            BC.check(V, None, V.tcr_ctx_create(0, C.byref(hv)))
            variant = (V, hv)
        kw = dict(ck_cd=1.0, r_out_km=R_OUT, substeps=1, thresholds=THR, n_groups=n_years, engine=eng)

        def wind(x, y, plane):
            return windfield.site_wind(dt[0], dt[1], dt[2], dt[3:], groups, x, y, DT, return_max=plane, **kw)

        for name, (slon, slat) in sites:
            tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
            order = sitescan.spatial_order(tl, ta, torch)
            sl, sa = tl[order].contiguous(), ta[order].contiguous()
            n_site = len(slon)
            cuts = list(range(0, n_site, block)) + [n_site]

            # (a) the select alone on the middle block, and the scan of that block with and without the plane
            b = (len(cuts) - 1) // 2
            i, j = cuts[b], cuts[b + 1]
            bl, ba = sl[i:j].contiguous(), sa[i:j].contiguous()
            counts = torch.empty((j - i, n_years, THR.size), dtype=torch.int32, device=dev)
            plane = torch.empty((j - i, n_trk), dtype=torch.float64, device=dev)
            level = torch.empty((j - i, k.size), dtype=torch.float64, device=dev)
            valid = torch.empty(j - i, dtype=torch.int32, device=dev)

            def scan_block(out):
                BC.check(L, h, L.tcr_windfield_dev(h, C.byref(wtrk), C.byref(wprm), j - i, bl.data_ptr(), ba.data_ptr(), THR.size,
                                                   THR.ctypes.data_as(_lib.DP), counts.data_ptr(), out, C.c_void_p(st.cuda_stream)))

            def select_block():
                BC.check(L, h, L.tcr_select_dev(h, plane.data_ptr(), j - i, n_trk, n_trk, k.size, ranks, level.data_ptr(), valid.data_ptr(),
                                                C.c_void_p(st.cuda_stream)))
            scan_ms, scan_runs = BC.timed(lambda: scan_block(None), st)
            fill_ms, fill_runs = BC.timed(lambda: scan_block(plane.data_ptr()), st)
            sel_ms, sel_runs = BC.timed(select_block, st)
            nv = valid.cpu().numpy()
            rows = np.unique(np.concatenate([[0, j - i - 1], np.argsort(nv)[[0, (j - i) // 2, -1]]]))
            want, want_valid = LN.row_select(plane[torch.as_tensor(rows, device=dev)].cpu().numpy(), k)
            assert LN.same_bits(level.cpu().numpy()[rows], want) and np.array_equal(nv[rows], want_valid), 'select != restatement'
            nbytes = (j - i) * n_trk * 8
            emit(what='(a) k_row_select alone', workload=name, block_rows=j - i, n_col=n_trk, ranks=k.tolist(), plane_bytes=nbytes,
                 select_ms=round(sel_ms, 3), select_ms_runs=[round(x, 3) for x in sel_runs],
                 plane_tb_per_s=round(nbytes / sel_ms / 1e9, 3), share_of_8_tb_per_s=round(nbytes / sel_ms / 1e9 / HBM_TBS, 3),
                 reach_min=int(nv.min()), reach_median=float(np.median(nv)), reach_max=int(nv.max()),
                 rows_on_global_path=round(float((nv > _lib.SELECT_LDS_KEYS).mean()), 4), lds_keys=_lib.SELECT_LDS_KEYS,
                 scan_of_the_block_ms=round(scan_ms, 3), scan_ms_runs=[round(x, 3) for x in scan_runs],
                 scan_with_plane_ms=round(fill_ms, 3), scan_with_plane_ms_runs=[round(x, 3) for x in fill_runs],
                 select_over_scan_of_its_block=round(sel_ms / scan_ms, 3), rows_checked_against_restatement=len(rows))
            del plane, level, valid, counts

            # (b) the blocked pass against the plain call, and the same blocks three ways
            res = {}

            def plain():
                res['plain'] = wind(tl, ta, False)

            def per_block(with_plane):
                for a, z in zip(cuts[:-1], cuts[1:]):
                    wind(sl[a:z], sa[a:z], with_plane)

            def driver(max_bytes=MAX_BYTES):
                res['levels'] = levels.site_return_levels(lambda x, y: wind(x, y, True), tl, ta, n_years, T, max_bytes=max_bytes,
                                                          n_trk=n_trk, engine=eng)
            plain_ms, plain_runs = host_timed(plain)
            nop_ms, nop_runs = host_timed(lambda: per_block(False))
            pl_ms, pl_runs = host_timed(lambda: per_block(True))
            drv_ms, drv_runs = host_timed(driver)
            assert torch.equal(res['levels']['counts'], res['plain']['counts']), 'blocked counts != plain counts'
            reach = res['levels']['n_reach'].cpu().numpy()
            r3 = lambda xs: [round(x, 2) for x in xs]                                       # noqa: E731
            emit(what='(b) site_return_levels over site_wind', workload=name, sites=n_site, tracks=n_trk, samples=lon.shape[1],
                 return_periods=list(T), ranks=k.tolist(), max_bytes=MAX_BYTES, block_sites=block, blocks=len(cuts) - 1,
                 plane_bytes_total=n_site * n_trk * 8, plain_site_wind_ms=round(plain_ms, 2), plain_ms_runs=r3(plain_runs),
                 blocked_levels_ms=round(drv_ms, 2), blocked_ms_runs=r3(drv_runs), ratio=round(drv_ms / plain_ms, 3),
                 blocks_without_plane_ms=round(nop_ms, 2), blocks_without_plane_ms_runs=r3(nop_runs),
                 blocks_with_plane_ms=round(pl_ms, 2), blocks_with_plane_ms_runs=r3(pl_runs),
                 overhead_blocking_ms=round(nop_ms - plain_ms, 2), overhead_plane_write_and_copy_back_ms=round(pl_ms - nop_ms, 2),
                 overhead_select_and_bookkeeping_ms=round(drv_ms - pl_ms, 2),
                 reach_min=int(reach.min()), reach_median=float(np.median(reach)), reach_max=int(reach.max()),
                 sites_with_a_10_year_level=int((~torch.isnan(res['levels']['return_level'][:, 0])).sum()),
                 check='blocked counts == plain counts; select == restatement on the rows checked in (a)')
            # the same pass with a larger budget for the plane: fewer blocks, fewer repeats of the scan's per-call work
            first, fewest = res['levels'], len(cuts) - 1
            for max_bytes in (2 ** 33, 2 ** 35):
                n_block = max(64, max_bytes // (8 * n_trk)) // 64 * 64
                if -(-n_site // n_block) >= fewest:
                    continue                                   # (no fewer blocks than with the budget before)
                fewest = -(-n_site // n_block)
                big_ms, big_runs = host_timed(lambda: driver(max_bytes))
                same = all(torch.equal(res['levels'][key].view(torch.int64) if key == 'return_level' else res['levels'][key],
                                       first[key].view(torch.int64) if key == 'return_level' else first[key])
                           for key in ('return_level', 'n_reach', 'counts'))
                assert same, 'the result depends on max_bytes'
                emit(what='(b) site_return_levels over site_wind', workload=name, sites=n_site, tracks=n_trk, max_bytes=max_bytes,
                     block_sites=n_block, blocks=fewest, plain_site_wind_ms=round(plain_ms, 2),
                     blocked_levels_ms=round(big_ms, 2), blocked_ms_runs=r3(big_runs), ratio=round(big_ms / plain_ms, 3),
                     check='bit-identical to the pass with max_bytes = 2^31')

            # (c) the select on every block, this library against one with another TCR_SELECT_LDS_KEYS
            if variant is None:
                continue
            blk_ms, share, same = {'this': [], 'variant': []}, [], True
            for i, j in zip(cuts[:-1], cuts[1:]):
                bl, ba = sl[i:j].contiguous(), sa[i:j].contiguous()
                counts = torch.empty((j - i, n_years, THR.size), dtype=torch.int32, device=dev)
                plane = torch.empty((j - i, n_trk), dtype=torch.float64, device=dev)
                BC.check(L, h, L.tcr_windfield_dev(h, C.byref(wtrk), C.byref(wprm), j - i, bl.data_ptr(), ba.data_ptr(), THR.size,
                                                   THR.ctypes.data_as(_lib.DP), counts.data_ptr(), plane.data_ptr(), C.c_void_p(st.cuda_stream)))
                out = {who: (torch.empty((j - i, k.size), dtype=torch.float64, device=dev), torch.empty(j - i, dtype=torch.int32, device=dev))
                       for who in blk_ms}
                runs = {who: [] for who in blk_ms}
                for _ in range(2):                                      # the two alternate: 6 runs each
                    for who, (lib, hh) in (('this', (L, h)), ('variant', variant)):
                        level, valid = out[who]
                        runs[who] += BC.timed(lambda: BC.check(lib, hh, lib.tcr_select_dev(
                            hh, plane.data_ptr(), j - i, n_trk, n_trk, k.size, ranks, level.data_ptr(), valid.data_ptr(),
                            C.c_void_p(st.cuda_stream))), st)[1]
                for who in blk_ms:
                    blk_ms[who].append(round(float(np.median(runs[who])), 3))
                same = same and torch.equal(out['this'][0].view(torch.int64), out['variant'][0].view(torch.int64)) and \
                    torch.equal(out['this'][1], out['variant'][1])
                share.append(round(float((out['this'][1] > _lib.SELECT_LDS_KEYS).float().mean()), 3))
            emit(what='(c) k_row_select on every block: TCR_SELECT_LDS_KEYS %d (this library) against the variant library'
                 % _lib.SELECT_LDS_KEYS, workload=name, blocks=len(cuts) - 1, this_ms_per_block=blk_ms['this'],
                 variant_ms_per_block=blk_ms['variant'], rows_over_lds_keys_per_block=share,
                 this_total_ms=round(sum(blk_ms['this']), 3), variant_total_ms=round(sum(blk_ms['variant']), 3), same_results=same)
        if variant is not None:
            variant[0].tcr_ctx_destroy(variant[1])
    if not quick:
        with open(out_fn, 'w') as f:
            f.write('\n'.join(lines) + '\n')


TAIL_PERIODS = (100.0, 250.0, 500.0, 1000.0)


def tail_main(args):
    quick = '--quick' in args
    K = int(args[args.index('--tail') + 1])
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'tail_levels_bench.txt')
    lines = []

    def emit(**row):
        text = json.dumps(row)
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(SEED)
    n_years, per_year, n_coast = BC.sizes(quick)
    lon, lat, v, env, groups = BC.make_storms(rng, n_years, per_year)
    sites = (('coast', BC.coast_sites(rng, n_coast)), ('grid', BC.grid_sites()))
    n_trk = lon.shape[0]
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    wtrk = BC.wind_tracks(dt, groups)
    wprm = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=R_OUT, rmax_const_km=0.0, substeps=1)
    T = np.array(TAIL_PERIODS)
    ranks = (C.c_int64 * 1)(K + 1)
    st = torch.cuda.current_stream(dev)
    block = max(64, MAX_BYTES // (8 * n_trk)) // 64 * 64
    with BC.open_context() as (L, h):
        eng = types.SimpleNamespace(h=h)
        parent = None
        if '--parent-lib' in args:
            V = C.CDLL(os.path.abspath(args[args.index('--parent-lib') + 1]))
            V.tcr_last_error.restype = C.c_char_p
            V.tcr_last_error.argtypes = [C.c_void_p]
            V.tcr_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
            V.tcr_ctx_destroy.argtypes = [C.c_void_p]
            V.tcr_select_dev.argtypes = L.tcr_select_dev.argtypes
            assert not hasattr(V, 'tcr_tail_dev'), 'the parent library already has the tail fit'
            hv = C.c_void_p()
            BC.check(V, None, V.tcr_ctx_create(0, C.byref(hv)))
            parent = (V, hv)
        kw = dict(ck_cd=1.0, r_out_km=R_OUT, substeps=1, thresholds=THR, n_groups=n_years, engine=eng)
        for name, (slon, slat) in sites:
            tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
            order = sitescan.spatial_order(tl, ta, torch)
            sl, sa = tl[order].contiguous(), ta[order].contiguous()
            n_site = len(slon)
            cuts = list(range(0, n_site, block)) + [n_site]

            # (d) the tail alone and the select alone on the middle block
            b = (len(cuts) - 1) // 2
            i, j = cuts[b], cuts[b + 1]
            bl, ba = sl[i:j].contiguous(), sa[i:j].contiguous()
            counts = torch.empty((j - i, n_years, THR.size), dtype=torch.int32, device=dev)
            plane = torch.empty((j - i, n_trk), dtype=torch.float64, device=dev)
            param = torch.empty((j - i, 3), dtype=torch.float64, device=dev)
            level = torch.empty((j - i, T.size), dtype=torch.float64, device=dev)
            valid = torch.empty(j - i, dtype=torch.int32, device=dev)
            sel = {who: torch.empty((j - i, 1), dtype=torch.float64, device=dev) for who in ('this', 'parent')}

            def scan_block(out):
                BC.check(L, h, L.tcr_windfield_dev(h, C.byref(wtrk), C.byref(wprm), j - i, bl.data_ptr(), ba.data_ptr(), THR.size,
                                                   THR.ctypes.data_as(_lib.DP), counts.data_ptr(), out, C.c_void_p(st.cuda_stream)))

            def select_block(lib, hh, out):
                BC.check(lib, hh, lib.tcr_select_dev(hh, plane.data_ptr(), j - i, n_trk, n_trk, 1, ranks, out.data_ptr(), valid.data_ptr(),
                                                     C.c_void_p(st.cuda_stream)))

            def tail_block():
                BC.check(L, h, L.tcr_tail_dev(h, plane.data_ptr(), j - i, n_trk, n_trk, K, float(n_years), T.size, T.ctypes.data_as(_lib.DP),
                                              param.data_ptr(), level.data_ptr(), valid.data_ptr(), C.c_void_p(st.cuda_stream)))
            scan_ms, scan_runs = BC.timed(lambda: scan_block(None), st)
            scan_block(plane.data_ptr())
            sel_ms, sel_runs = BC.timed(lambda: select_block(L, h, sel['this']), st)
            row = {}
            if parent is not None:
                par_ms, par_runs = BC.timed(lambda: select_block(parent[0], parent[1], sel['parent']), st)
                again_ms, again_runs = BC.timed(lambda: select_block(L, h, sel['this']), st)
                assert torch.equal(sel['this'].view(torch.int64), sel['parent'].view(torch.int64)), 'select: this library != parent library'
                row = dict(parent_select_ms=round(par_ms, 3), parent_select_ms_runs=[round(x, 3) for x in par_runs],
                           select_again_ms=round(again_ms, 3), select_again_ms_runs=[round(x, 3) for x in again_runs],
                           select_this_over_parent=round(min(sel_ms, again_ms) / par_ms, 3))
            tail_ms, tail_runs = BC.timed(tail_block, st)
            nv = valid.cpu().numpy()
            fitted = ~torch.isnan(param[:, 1]).cpu().numpy()
            rows = np.unique(np.concatenate([[0, j - i - 1], np.argsort(nv)[[0, (j - i) // 4, (j - i) // 2, 3 * (j - i) // 4, -1]]]))
            want = TN.row_tail(plane[torch.as_tensor(rows, device=dev)].cpu().numpy(), K, n_years, T)
            got = dict(threshold=param[:, 0], xi=param[:, 1], sigma=param[:, 2], level=level, n_valid=valid)
            got = {key: a.cpu().numpy()[rows] for key, a in got.items()}
            for key in ('threshold', 'xi', 'sigma'):
                assert LN.same_bits(got[key], want[key]), 'tail != restatement: ' + key
            assert np.array_equal(got['n_valid'], want['n_valid']) and np.array_equal(np.isnan(got['level']), np.isnan(want['level']))
            assert LN.same_bits(param[:, 0].cpu().numpy(), sel['this'][:, 0].cpu().numpy()), 'threshold != select of rank K + 1'
            with np.errstate(invalid='ignore', divide='ignore'):
                err = np.abs(got['level'] - want['level']) / (np.abs(want['threshold'][:, None]) + np.abs(want['level'] - want['threshold'][:, None]))
            err = float(np.nanmax(err)) if np.isfinite(err).any() else 0.0
            assert err <= 1e-13, err
            xi = param[:, 1].cpu().numpy()[fitted]
            nbytes = (j - i) * n_trk * 8
            emit(what='(d) k_row_tail alone against k_row_select alone (one rank, K + 1)', workload=name, block_rows=j - i, n_col=n_trk,
                 exceedances=K, return_periods=list(TAIL_PERIODS), total_years=n_years, plane_bytes=nbytes,
                 tail_ms=round(tail_ms, 3), tail_ms_runs=[round(x, 3) for x in tail_runs],
                 select_ms=round(sel_ms, 3), select_ms_runs=[round(x, 3) for x in sel_runs], **row,
                 tail_over_select=round(tail_ms / sel_ms, 3), scan_of_the_block_ms=round(scan_ms, 3),
                 scan_ms_runs=[round(x, 3) for x in scan_runs], tail_over_scan_of_its_block=round(tail_ms / scan_ms, 3),
                 select_over_scan_of_its_block=round(sel_ms / scan_ms, 3), plane_tb_per_s=round(nbytes / tail_ms / 1e9, 3),
                 reach_min=int(nv.min()), reach_median=float(np.median(nv)), reach_max=int(nv.max()),
                 rows_on_global_path=round(float((nv > _lib.SELECT_LDS_KEYS).mean()), 4), rows_with_a_threshold=int((nv >= K + 1).sum()),
                 rows_with_a_fit=int(fitted.sum()), xi_min=round(float(xi.min()), 4) if xi.size else None,
                 xi_median=round(float(np.median(xi)), 4) if xi.size else None, xi_max=round(float(xi.max()), 4) if xi.size else None,
                 rows_checked_against_restatement=len(rows), max_level_error_over_u_plus_excess=err)
            del plane, level, valid, counts, param

            # (e) the blocked pass at one block, with and without the tail
            res = {}

            def driver(tail):
                res[tail] = levels.site_return_levels(
                    lambda x, y: windfield.site_wind(dt[0], dt[1], dt[2], dt[3:], groups, x, y, DT, return_max=True, **kw), tl, ta, n_years,
                    TAIL_PERIODS, max_bytes=2 ** 35, n_trk=n_trk, engine=eng, tail_exceedances=tail)
            plain_ms, plain_runs = host_timed(lambda: driver(None))
            with_ms, with_runs = host_timed(lambda: driver(K))
            for key in ('return_level', 'n_reach', 'counts'):
                a_, b_ = res[None][key], res[K][key]
                assert torch.equal(a_.view(torch.int64) if key == 'return_level' else a_, b_.view(torch.int64) if key == 'return_level' else b_), key
            lv = res[K]['tail_level']
            emit(what='(e) site_return_levels over site_wind at one block, with and without tail_exceedances', workload=name, sites=n_site,
                 tracks=n_trk, exceedances=K, return_periods=list(TAIL_PERIODS), max_bytes=2 ** 35,
                 blocks=-(-n_site // (max(64, 2 ** 35 // (8 * n_trk)) // 64 * 64)),
                 without_tail_ms=round(plain_ms, 2), without_tail_ms_runs=[round(x, 2) for x in plain_runs],
                 with_tail_ms=round(with_ms, 2), with_tail_ms_runs=[round(x, 2) for x in with_runs], ratio=round(with_ms / plain_ms, 3),
                 sites_with_a_1000_year_tail_level=int((~torch.isnan(lv[:, -1])).sum()),
                 sites_with_a_1000_year_order_statistic=int((~torch.isnan(res[K]['return_level'][:, -1])).sum()),
                 check='return_level, n_reach and counts are the same bits with and without the tail')
        if parent is not None:
            parent[0].tcr_ctx_destroy(parent[1])
    if not quick:
        with open(out_fn, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    if '--tail' in sys.argv[1:]:
        tail_main(sys.argv[1:])
    else:
        main()
