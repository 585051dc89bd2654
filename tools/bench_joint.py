"""Cost of the joint site hazard (joint.py, csrc/tcr_joint.hip) on tools/bench_windfield.py's tracks (bench_common; 45 000 tracks x 361
samples, r_out = 500 km, substeps 1), the 0.25-degree NA grid (87 001 sites) and the `coast` set (10 000 sites), the wind
footprint, levels 17.5 and 33 m/s, one bit per storm.

Reports, every run listed beside its median, the variants of a part taken in turn in a random order per round:

  (a) the blocked footprint pass (levels.site_blocks over windfield.site_wind with its plane on, max_bytes = 2^31) with every plane
      only dropped, against the same pass with every plane packed into the bit table (joint.pack_bits), 3 rounds after a warm-up
      (host clock around work that ends in a device synchronise; one library context for all);
  (b) k_joint_pack alone (tcr_joint_pack_dev, both levels) on the plane of the block in the middle of the spatial order, against a
      device-to-device copy of the same plane, the yardstick of profiles/event_table_bench.txt, by device events, 5 rounds.  The
      pack reads the plane once and writes 1/64 of it per level, the copy moves twice its bytes.  A few rows are compared with the
      restatement (tests/joint_numpy.py);
  (c) tcr_joint_cross_dev for 100 anchors x all grid sites and for the coast set against itself, both levels, by device events, 5
      rounds, against the route a user would write today with torch on the boolean plane E [site][storm]: (E_a.half() @ E.half().T)
      per level, and torch._int_mm on int8 where the installed torch offers it on this device (noted when it does not).  The
      boolean planes are unpacked from the bit table beforehand and are not part of the timing; what the torch routes return is
      compared with the counts (fp16 cannot hold every count above 2048 exactly: reported, not asserted).  joint_over_torch is the
      ratio of the medians.

No ratio is fixed in advance: the record holds what was measured, and the commit whose library it was measured with (git describe,
or --built-from where the tree is not a checkout).

    python tools/bench_joint.py [--quick] [--out profiles/joint_bench.txt] [--built-from TEXT]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time
import types

import numpy as np

import bench_common as BC
from bench_common import ROOT
import torch  # noqa: E402  (importing it does not touch the GPU)
from tests import joint_numpy as JN  # noqa: E402
from tropical_cyclone_risk_amd import joint, levels, sitescan, windfield  # noqa: E402

SEED = 7
R_OUT = 500.0
DT = 3600.0
MAX_BYTES = 2 ** 31
LEVELS = np.array([17.5, 33.0])
THR = np.concatenate([[17.5], np.arange(20.0, 81.0, 5.0)])
N_ANCHOR = 100


def shuffled(fns, order_rng, stream=None, K=3):
    """{name: runs in ms} of the functions, K rounds after a warm-up round, in a random order per round; by device events on
    `stream`, or (None) by the host clock around work that ends in a device synchronise."""
    runs = {name: [] for name in fns}
    for name in fns:
        fns[name]()
    torch.cuda.synchronize()
    for _ in range(K):
        for name in order_rng.permutation(list(fns)):
            fn = fns[name]
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


def unpack_rows(bits, n_unit, dtype):
    """[n_row][n_unit] of `dtype` (0 / 1) from bit rows [n_row][n_word] int64, on the device."""
    shifts = torch.arange(64, dtype=torch.int64, device=bits.device)
    out = torch.empty((bits.shape[0], n_unit), dtype=dtype, device=bits.device)
    for i in range(0, int(bits.shape[0]), 4096):
        e = (bits[i:i + 4096, :, None] >> shifts) & 1
        out[i:i + 4096] = e.reshape(e.shape[0], -1)[:, :n_unit].to(dtype)
    return out


def main():
    args = sys.argv[1:]
    quick = '--quick' in args
    out_fn = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'joint_bench.txt')
    lines = []

    def emit(**row):
        text = json.dumps(row)
        print(text, flush=True)
        lines.append(text)
    med = lambda xs: round(float(np.median(xs)), 3)                                 # noqa: E731
    r3 = lambda xs: [round(float(x), 3) for x in xs]                                # noqa: E731

    rng = np.random.default_rng(SEED)
    order_rng = np.random.default_rng(SEED + 1)
    n_years, per_year, n_coast = BC.sizes(quick)
    lon, lat, v, env, groups = BC.make_storms(rng, n_years, per_year)
    clon, clat = BC.coast_sites(rng, n_coast)
    slon, slat = BC.grid_sites()
    if quick:
        slon, slat = slon[::7], slat[::7]
    n_trk, n_site = lon.shape[0], len(slon)
    dev = torch.device('cuda', 0)
    dt = [torch.as_tensor(a, device=dev) for a in [lon, lat, v] + env]
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    if '--built-from' in args:                         # (where the tree is not a checkout)
        built = args[args.index('--built-from') + 1]
    else:
        try:
            built = subprocess.check_output(['git', 'describe', '--always', '--dirty'], cwd=ROOT, text=True, stderr=subprocess.DEVNULL).strip()
        except (OSError, subprocess.CalledProcessError):
            built = 'unknown'
    emit(what='library', built_from=built, tracks=n_trk, samples=lon.shape[1],
         grid_sites=n_site, coast_sites=n_coast, levels=LEVELS.tolist(), unit='storm')
    tl, ta = torch.as_tensor(slon, device=dev), torch.as_tensor(slat, device=dev)
    tcl, tca = torch.as_tensor(clon, device=dev), torch.as_tensor(clat, device=dev)
    with BC.open_context() as (L, h):
        eng = types.SimpleNamespace(h=h)
        kw = dict(ck_cd=1.0, r_out_km=R_OUT, substeps=1, thresholds=THR, n_groups=n_years, engine=eng)

        def wind(x, y):
            return windfield.site_wind(dt[0], dt[1], dt[2], dt[3:], groups, x, y, DT, return_max=True, **kw)
        n_word = (n_trk + 63) // 64
        keep = {}

        def blocks(x, y):
            fl, a, o, mb = levels.check_sites(x, y, MAX_BYTES)
            return levels.site_blocks(wind, fl, a, o, 'site_max', mb, n_trk)

        def dropped():
            for _, _, p, r, _ in blocks(tl, ta):
                del p, r

        def packed(x=tl, y=ta, name='grid'):
            table = torch.empty((LEVELS.size, int(x.shape[0]), n_word), dtype=torch.int64, device=dev)
            n_set = torch.empty((LEVELS.size, int(x.shape[0])), dtype=torch.int32, device=dev)
            for i, j, p, r, _ in blocks(x, y):
                table[:, i:j], n_set[:, i:j] = joint.pack_bits(p, LEVELS, engine=eng)
                del p, r
            keep[name] = table, n_set

        # (a) the blocked pass with the planes dropped against the same pass with the planes packed
        runs = shuffled(dict(dropped=dropped, packed=packed), order_rng)
        block = max(64, MAX_BYTES // (8 * n_trk)) // 64 * 64
        dm, pm = med(runs['dropped']), med(runs['packed'])
        emit(what='(a) blocked site_wind pass with the planes dropped against the same pass with the planes packed, 2 levels', sites=n_site,
             block_sites=block, blocks=-(-n_site // block), table_bytes=int(LEVELS.size) * n_site * n_word * 8, dense_bytes=8 * n_site * n_trk,
             planes_dropped_ms=dm, planes_dropped_ms_runs=r3(runs['dropped']), planes_packed_ms=pm, planes_packed_ms_runs=r3(runs['packed']),
             ratio=round(pm / dm, 3), bits_set_share=[round(float(keep['grid'][1][l].sum()) / (n_site * n_trk), 5) for l in range(LEVELS.size)])

        # (b) the pack kernel alone on the middle block's plane, against a copy of it
        order = sitescan.spatial_order(tl, ta, torch)
        sl, sa = tl[order].contiguous(), ta[order].contiguous()
        cuts = list(range(0, n_site, block)) + [n_site]
        b = (len(cuts) - 1) // 2
        i, j = cuts[b], cuts[b + 1]
        n_row = j - i
        plane = wind(sl[i:j], sa[i:j])['site_max'].contiguous()
        other = torch.empty_like(plane)
        lev = torch.as_tensor(np.repeat(LEVELS[None, :], n_row, axis=0), device=dev)
        bits = torch.empty((LEVELS.size, n_row, n_word), dtype=torch.int64, device=dev)
        n_set = torch.empty((LEVELS.size, n_row), dtype=torch.int32, device=dev)

        def pack():
            BC.check(L, h, L.tcr_joint_pack_dev(h, plane.data_ptr(), n_row, n_trk, n_trk, lev.data_ptr(), int(LEVELS.size), None, n_trk,
                                                bits.data_ptr(), n_row * n_word, n_set.data_ptr(), n_row, sp))
        runs = shuffled(dict(pack=pack, copy=lambda: other.copy_(plane)), order_rng, st, K=5)
        rows = np.unique([0, n_row // 2, n_row - 1, int(n_set[0].argmax())])
        hb, hs = bits.cpu().numpy().view(np.uint64), n_set.cpu().numpy()
        for r in rows:
            wb, ws = JN.pack_bits(plane[int(r)].cpu().numpy()[None, :], LEVELS)
            assert np.array_equal(hb[:, r], wb[:, 0]) and np.array_equal(hs[:, r], ws[:, 0]), 'pack_bits != restatement'
        nbytes = n_row * n_trk * 8
        km, cm = med(runs['pack']), med(runs['copy'])
        emit(what='(b) tcr_joint_pack_dev alone (2 levels) against a device-to-device copy of the plane', block_rows=n_row, n_col=n_trk,
             plane_bytes=nbytes, bits_bytes=int(LEVELS.size) * n_row * n_word * 8, pack_ms=km, pack_ms_runs=r3(runs['pack']), copy_ms=cm,
             copy_ms_runs=r3(runs['copy']), pack_over_copy=round(km / cm, 3), pack_read_tb_per_s=round(nbytes / km / 1e9, 3),
             copy_read_plus_write_tb_per_s=round(2 * nbytes / cm / 1e9, 3), rows_checked_against_restatement=len(rows))
        del plane, other, bits, n_set, lev

        # (c) the cross against torch on the boolean plane
        packed(tcl, tca, 'coast')
        grid, coast = keep['grid'][0], keep['coast'][0]
        busiest = torch.argsort(keep['grid'][1][0], descending=True)[:N_ANCHOR]
        cases = (('100 anchors x all grid sites', grid[:, busiest].contiguous(), grid),
                 ('coast x coast', coast, coast))
        for name, a, bt in cases:
            n_a, n_b = int(a.shape[1]), int(bt.shape[1])
            counts = torch.empty((LEVELS.size, n_a, n_b), dtype=torch.int32, device=dev)

            def cross():
                BC.check(L, h, L.tcr_joint_cross_dev(h, a.data_ptr(), n_a, n_a * n_word, bt.data_ptr(), n_b, n_b * n_word, n_word, int(LEVELS.size),
                                                     counts.data_ptr(), sp))
            fns, outs, notes = dict(joint_cross=cross), {}, {}
            ea16 = [unpack_rows(a[l], n_trk, torch.float16) for l in range(LEVELS.size)]
            eb16 = [ea16[l] if bt is a else unpack_rows(bt[l], n_trk, torch.float16) for l in range(LEVELS.size)]

            def half():
                outs['torch_fp16'] = [ea16[l] @ eb16[l].T for l in range(LEVELS.size)]
            fns['torch_fp16'] = half
            if hasattr(torch, '_int_mm'):
                try:
                    k8 = (n_trk + 7) // 8 * 8                       # (torch._int_mm wants the inner size a multiple of 8)
                    n8 = (n_b + 7) // 8 * 8                         # (and the columns of the result)
                    ea8 = [torch.nn.functional.pad(e.to(torch.int8), (0, k8 - n_trk)) for e in ea16]
                    eb8 = [torch.nn.functional.pad(e.to(torch.int8), (0, k8 - n_trk, 0, n8 - n_b)) for e in eb16]

                    def int8():
                        outs['torch_int8'] = [torch._int_mm(ea8[l], eb8[l].T)[:, :n_b] for l in range(LEVELS.size)]
                    int8()
                    torch.cuda.synchronize()
                    fns['torch_int8'] = int8
                except Exception as e:                              # noqa: BLE001  (whatever this torch says about this device)
                    notes['torch_int8'] = 'not offered here: %s' % str(e).splitlines()[0][:200]
            else:
                notes['torch_int8'] = 'this torch has no torch._int_mm'
            runs = shuffled(fns, order_rng, st, K=5)
            want = counts.cpu().numpy()
            probe = np.unique([0, n_a // 2, n_a - 1])
            ref = JN.cross_counts(a[:, probe].cpu().numpy(), bt[:, :2048].cpu().numpy())
            assert np.array_equal(want[:, probe, :2048], ref), 'cross_counts != restatement'
            row = dict(what='(c) tcr_joint_cross_dev against torch on the boolean plane: ' + name, n_a=n_a, n_b=n_b, n_word=n_word, levels=int(LEVELS.size),
                       bits_bytes=int((a.numel() + (0 if bt is a else bt.numel())) * 8), max_count=int(want.max()), cells_checked_against_restatement=int(ref.size))
            jm = med(runs['joint_cross'])
            row.update(joint_cross_ms=jm, joint_cross_ms_runs=r3(runs['joint_cross']),
                       cell_words_per_ns=round(LEVELS.size * n_a * n_b * n_word / jm / 1e6, 1))
            for who in ('torch_fp16', 'torch_int8'):
                if who in runs:
                    got = np.stack([o.cpu().numpy().astype(np.int64) for o in outs[who]])
                    row.update({who + '_ms': med(runs[who]), who + '_ms_runs': r3(runs[who]), who + '_exact': bool(np.array_equal(got, want)),
                                who + '_operand_bytes': int(sum(e.numel() * e.element_size() for e in (ea16 + ([] if bt is a else eb16)))
                                                            // (1 if who == 'torch_fp16' else 2)),
                                'joint_over_' + who: round(jm / med(runs[who]), 3)})
                else:
                    row[who] = notes[who]
            row['joint_over_torch'] = max(row[k] for k in row if k.startswith('joint_over_torch_'))        # (against the faster of them)
            emit(**row)
            del ea16, eb16, counts
    if not quick:
        if os.path.exists(out_fn):                     # the compiler's resource report of the kernels is kept (it is not a run's)
            lines += [t.rstrip('\n') for t in open(out_fn) if t.startswith('{"what": "kernel resources')]
        with open(out_fn, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
