"""Cost of event footprints (events.py, csrc/tcr_rowpack.hip) on tools/bench_windfield.py's tracks (bench_common; 45 000 tracks x 361
samples, r_out = 500 km, substeps 1) and the 0.25-degree NA grid (87 001 sites), the wind footprint, floors 17.5 and 33 m/s.

Reports, every run listed beside its median:

  (a) the kernels alone on one block's plane, the block of the middle of the spatial order as events.site_event_table cuts it
      (max_bytes = 2^31) and the wind footprint fills it, by device events: tcr_rowpack_count_dev (k_rowpack_count and the scan of
      the row counts), tcr_rowpack_fill_dev (k_rowpack_fill) and a device-to-device copy of the same plane, the three alternating, 5
      rounds after a warm-up.  The count reads the plane once, the fill reads it once and writes a few per cent of it, the copy moves
      twice those bytes: each kernel is expected to take no longer than the copy.  A few rows are compared with the restatement
      (tests/events_numpy.py);
  (b) the blocked events.site_event_table pass against the same blocked pass (levels.site_blocks over windfield.site_wind with its
      plane on) with every plane only dropped, the two alternating, 3 rounds after a warm-up (host clock around work that ends in a
      device synchronise; one library context for all), at max_bytes = 2^31 and 2^35 (one block): the ratio, nnz, and the table's
      bytes (12 per entry and 8 per site) against the dense matrix's.  The tables of the two block sizes must be the same bits, and
      counts_from_table at the floor 17.5 = a threshold of its own must give the scan's counts from that threshold on;
  (c) with --parent-lib: tcr_windfield_dev with the plane on every block, this tree's library against a library built from the
      parent commit, the two alternating, 3 rounds: the scan is the parent's code, and (b)'s baseline is therefore the parent's.

The record's last line is the compiler's resource report of the three kernels (`python tools/kernel_resources.py --grep rowpack`),
written by hand and kept across runs.

    python tools/bench_events.py [--parent-lib PATH/libtcrisk_hip.so] [--quick] [--out profiles/event_table_bench.txt]
"""
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np

import bench_common as BC
from bench_common import ROOT
import torch  # noqa: E402  (importing it does not touch the GPU)
from tests import events_numpy as EN  # noqa: E402
from tests.levels_numpy import same_bits  # noqa: E402
from tropical_cyclone_risk_amd import _lib, events, levels, sitescan, windfield  # noqa: E402

SEED = 7
R_OUT = 500.0
DT = 3600.0
MAX_BYTES = 2 ** 31
FLOORS = (17.5, 33.0)
THR = np.concatenate([[17.5], np.arange(20.0, 81.0, 5.0)])         # (the first floor is a threshold: counts_from_table has its check)


def alternating(fns, stream=None, K=3):
    """{name: runs in ms} of the functions taken in turn, K rounds after a warm-up round; by device events on `stream`, or (None) by
    the host clock around work that ends in a device synchronise."""
    runs = {name: [] for name in fns}
    for name in fns:
        fns[name]()
    torch.cuda.synchronize()
    for _ in range(K):
        for name, fn in fns.items():
            if stream is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream); fn(); e1.record(stream)
                torch.cuda.synchronize()
                runs[name].append(e0.elapsed_time(e1))
            else:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                runs[name].append((time.perf_counter() - t0) * 1e3)
    return runs


def main():
    args = sys.argv[1:]
    quick = '--quick' in args
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'event_table_bench.txt')
    lines = []

    def emit(**row):
        text = json.dumps(row)
        print(text, flush=True)
        lines.append(text)
    med = lambda xs: round(float(np.median(xs)), 3)                                 # noqa: E731
    r3 = lambda xs: [round(float(x), 3) for x in xs]                                # noqa: E731

    rng = np.random.default_rng(SEED)
    n_years, per_year, _ = BC.sizes(quick)
    lon, lat, v, env, groups = BC.make_storms(rng, n_years, per_year)
    slon, slat = BC.grid_sites()
    if quick:
        slon, slat = slon[::7], slat[::7]
    n_trk, n_site = lon.shape[0], len(slon)
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    wtrk = BC.wind_tracks(dt, groups)
    wprm = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=R_OUT, rmax_const_km=0.0, substeps=1)
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    block = max(64, MAX_BYTES // (8 * n_trk)) // 64 * 64
    tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
    order = sitescan.spatial_order(tl, ta, torch)
    sl, sa = tl[order].contiguous(), ta[order].contiguous()
    cuts = list(range(0, n_site, block)) + [n_site]
    with BC.open_context() as (L, h):
        eng = types.SimpleNamespace(h=h)

        def scan_block(lib, hh, i, j, counts, plane):
            BC.check(lib, hh, lib.tcr_windfield_dev(hh, C.byref(wtrk), C.byref(wprm), j - i, sl[i:j].data_ptr(), sa[i:j].data_ptr(), THR.size,
                                                    THR.ctypes.data_as(_lib.DP), counts.data_ptr(), plane.data_ptr(), sp))

        # (a) the kernels alone on the middle block's plane, against a copy of it
        b = (len(cuts) - 1) // 2
        i, j = cuts[b], cuts[b + 1]
        n_row = j - i
        counts = torch.empty((n_row, n_years, THR.size), dtype=torch.int32, device=dev)
        plane = torch.empty((n_row, n_trk), dtype=torch.float64, device=dev)
        other = torch.empty_like(plane)
        scan_block(L, h, i, j, counts, plane)
        nbytes = n_row * n_trk * 8
        for floor in FLOORS:
            ptr = torch.empty(n_row + 1, dtype=torch.int64, device=dev)

            def count():
                BC.check(L, h, L.tcr_rowpack_count_dev(h, plane.data_ptr(), n_row, n_trk, n_trk, floor, ptr.data_ptr(), sp))
            count()
            nnz = int(ptr[n_row])
            col, val = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.float64, device=dev)

            def fill():
                BC.check(L, h, L.tcr_rowpack_fill_dev(h, plane.data_ptr(), n_row, n_trk, n_trk, floor, ptr.data_ptr(), nnz, col.data_ptr(),
                                                      val.data_ptr(), sp))
            runs = alternating(dict(count=count, fill=fill, copy=lambda: other.copy_(plane)), st, K=5)
            per_row = (ptr[1:] - ptr[:-1]).cpu().numpy()
            rows = np.unique(np.concatenate([[0, n_row - 1], np.argsort(per_row)[[0, n_row // 2, -1]]]))
            hp, hc, hv = ptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()
            for r in rows:
                _, wc, wv = EN.row_pack(plane[int(r)].cpu().numpy()[None, :], floor)
                assert np.array_equal(hc[hp[r]:hp[r + 1]], wc) and same_bits(hv[hp[r]:hp[r + 1]], wv), 'row_pack != restatement'
            cm, fm, pm = med(runs['count']), med(runs['fill']), med(runs['copy'])
            emit(what='(a) tcr_rowpack_count_dev and tcr_rowpack_fill_dev alone against a device-to-device copy of the plane',
                 min_value=floor, block_rows=n_row, n_col=n_trk, plane_bytes=nbytes, nnz=nnz, kept_share=round(nnz / (n_row * n_trk), 5),
                 not_nan_share=round(float((~torch.isnan(plane)).float().mean()), 5),
                 kept_per_row_min=int(per_row.min()), kept_per_row_median=float(np.median(per_row)), kept_per_row_max=int(per_row.max()),
                 count_ms=cm, count_ms_runs=r3(runs['count']), fill_ms=fm, fill_ms_runs=r3(runs['fill']),
                 copy_ms=pm, copy_ms_runs=r3(runs['copy']), count_over_copy=round(cm / pm, 3), fill_over_copy=round(fm / pm, 3),
                 count_read_tb_per_s=round(nbytes / cm / 1e9, 3), fill_read_tb_per_s=round(nbytes / fm / 1e9, 3),
                 copy_read_plus_write_tb_per_s=round(2 * nbytes / pm / 1e9, 3), rows_checked_against_restatement=len(rows))
            del col, val, ptr
        del plane, other, counts

        # (b) the event-table pass against the same blocked pass with the planes dropped
        kw = dict(ck_cd=1.0, r_out_km=R_OUT, substeps=1, thresholds=THR, n_groups=n_years, engine=eng)

        def wind(x, y, plane):
            return windfield.site_wind(dt[0], dt[1], dt[2], dt[3:], groups, x, y, DT, return_max=plane, **kw)
        res = {}

        def dropped(max_bytes):
            fl, a, o, mb = levels.check_sites(tl, ta, max_bytes)
            for _, _, p, r, _ in levels.site_blocks(lambda x, y: wind(x, y, True), fl, a, o, 'site_max', mb, n_trk):
                del p, r

        def table(floor, max_bytes):
            res[floor, max_bytes] = events.site_event_table(lambda x, y: wind(x, y, True), tl, ta, floor, max_bytes=max_bytes, n_trk=n_trk,
                                                            engine=eng)
        plain = alternating(dict(plain=lambda: res.__setitem__('plain', wind(tl, ta, False))))['plain']
        for max_bytes in (MAX_BYTES, 2 ** 35):
            n_block = max(64, max_bytes // (8 * n_trk)) // 64 * 64
            fns = dict(dropped=lambda: dropped(max_bytes))
            for floor in FLOORS:
                fns['table_%g' % floor] = (lambda f: lambda: table(f, max_bytes))(floor)
            runs = alternating(fns)
            for floor in FLOORS:
                t = res[floor, max_bytes]
                nnz = int(t['storm'].shape[0])
                per = (t['site_ptr'][1:] - t['site_ptr'][:-1]).cpu().numpy()
                tm, dm = med(runs['table_%g' % floor]), med(runs['dropped'])
                emit(what='(b) site_event_table over site_wind against the same blocks with the planes dropped', min_value=floor,
                     sites=n_site, tracks=n_trk, samples=lon.shape[1], max_bytes=max_bytes, block_sites=n_block, blocks=-(-n_site // n_block),
                     nnz=nnz, table_bytes=12 * nnz + 8 * (n_site + 1), dense_bytes=8 * n_site * n_trk,
                     table_over_dense=round((12 * nnz + 8 * (n_site + 1)) / (8 * n_site * n_trk), 5),
                     events_per_site_median=float(np.median(per)), events_per_site_max=int(per.max()), sites_without_events=int((per == 0).sum()),
                     event_table_ms=tm, event_table_ms_runs=r3(runs['table_%g' % floor]), planes_dropped_ms=dm,
                     planes_dropped_ms_runs=r3(runs['dropped']), ratio=round(tm / dm, 3), plain_site_wind_ms=med(plain),
                     plain_ms_runs=r3(plain), event_table_over_plain=round(tm / med(plain), 3))
        for floor in FLOORS:
            a_, b_ = res[floor, MAX_BYTES], res[floor, 2 ** 35]
            assert torch.equal(a_['site_ptr'], b_['site_ptr']) and torch.equal(a_['storm'], b_['storm']), 'the table depends on max_bytes'
            assert torch.equal(a_['value'].view(torch.int64), b_['value'].view(torch.int64)) and torch.equal(a_['counts'], b_['counts'])
        t = res[FLOORS[0], MAX_BYTES]
        assert torch.equal(t['counts'], res['plain']['counts']), 'blocked counts != plain counts'
        assert torch.equal(events.counts_from_table(t, groups, n_years, THR), t['counts']), 'counts_from_table != the scan\'s counts'
        k = int(np.searchsorted(THR, FLOORS[1]))
        assert THR[k] >= FLOORS[1]
        assert torch.equal(events.counts_from_table(res[FLOORS[1], MAX_BYTES], groups, n_years, THR[k:]), t['counts'][:, :, k:])
        emit(what='(b) checks', same_table_at_both_block_sizes=True, blocked_counts_equal_plain_counts=True,
             counts_from_table_equal_scan_counts=True)
        res.clear()

        # (c) the scan with its plane on every block: this library against the parent commit's
        if '--parent-lib' in args:
            V = C.CDLL(os.path.abspath(args[args.index('--parent-lib') + 1]))
            V.tcr_last_error.restype = C.c_char_p
            V.tcr_last_error.argtypes = [C.c_void_p]
            V.tcr_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
            V.tcr_ctx_destroy.argtypes = [C.c_void_p]
            V.tcr_windfield_dev.argtypes = L.tcr_windfield_dev.argtypes
            assert not hasattr(V, 'tcr_rowpack_host'), 'the parent library already has row packing'
            hv = C.c_void_p()
            BC.check(V, None, V.tcr_ctx_create(0, C.byref(hv)))
            counts = torch.empty((block, n_years, THR.size), dtype=torch.int32, device=dev)
            out = {who: torch.empty((block, n_trk), dtype=torch.float64, device=dev) for who in ('this', 'parent')}

            def all_blocks(lib, hh, plane):
                for a, z in zip(cuts[:-1], cuts[1:]):
                    scan_block(lib, hh, a, z, counts, plane)
            runs = alternating(dict(this=lambda: all_blocks(L, h, out['this']), parent=lambda: all_blocks(V, hv, out['parent'])), st)
            n_last = cuts[-1] - cuts[-2]
            same = torch.equal(out['this'][:n_last].view(torch.int64), out['parent'][:n_last].view(torch.int64))
            emit(what='(c) tcr_windfield_dev with its plane on every block: this library against the parent commit\'s', blocks=len(cuts) - 1,
                 this_ms=med(runs['this']), this_ms_runs=r3(runs['this']), parent_ms=med(runs['parent']), parent_ms_runs=r3(runs['parent']),
                 this_over_parent=round(med(runs['this']) / med(runs['parent']), 3), same_last_plane=same)
            V.tcr_ctx_destroy(hv)
    if not quick:
        if os.path.exists(out_fn):                     # the compiler's resource report of the kernels is kept (it is not a run's)
            lines += [t.rstrip('\n') for t in open(out_fn) if t.startswith('{"what": "kernel resources')]
        with open(out_fn, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
