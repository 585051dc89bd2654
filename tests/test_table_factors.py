"""The forcing table's phase factors formed inside the table kernel (tcr_tune.table_factors, the default) against the
separate k_phase_factors_frag launch (table_factors = 0).

Both paths evaluate one expression (tcr_kernels.hip: phase_factor) on the same phases and feed the same MFMAs in the same
order, so everything here is compared bit for bit.  The fused first-segment launch is also the batch's first kernel and
zeroes the batch's counters (BatchReset): the last test runs a round behind a round that leaves more behind.
"""
import os
import re

import numpy as np
import pytest

from tests.test_inflight_accept import B, B_ALL, COUNTERS, KEYS, N_CAND, YEAR_ALL, _pipe, _seeded

PLANTED = (0.0, 0.25, 0.5, 1.0 - 2.0 ** -53)


def test_table_kernel_register_budget():
    """Every k_fourier_mfma instantiation (fp64 / fp32, list or not, fused or not) keeps two waves per SIMD — at most 256
    VGPRs + AGPRs — without scratch, and the fallback's k_phase_factors_frag is still built.  From the compiler's resource
    report, as tests/test_abi.py::test_kernel_register_budgets reads it."""
    import subprocess
    from tropical_cyclone_risk_amd import build as Bd
    cmd = [Bd.hipcc()] + Bd.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-o', os.devnull, os.path.join(Bd.CSRC, 'tcr_abi.hip')]
    out = subprocess.run(cmd, cwd=Bd.CSRC, capture_output=True, text=True).stderr
    rows, cur = {}, None
    for line in out.splitlines():
        m = re.search(r'remark: \S+ +(Function Name|Name): (\S+)', line)
        if m:
            cur = rows.setdefault(m.group(2), {})
            continue
        m = re.search(r'(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)', line)
        if m and cur is not None:
            cur[m.group(1).split()[0]] = int(m.group(2))
    assert len(rows) > 40, 'no resource report from hipcc'
    table = {}
    for name, r in rows.items():
        m = re.match(r'_ZN3tcr14k_fourier_mfmaI([df])Lb([01])ELb([01])EEE', name)
        if m:
            table[m.groups()] = r
    want = {(t, l, f) for t in 'df' for l in '01' for f in '01'}
    assert set(table) == want, sorted(want - set(table))
    for key, r in sorted(table.items()):
        print('k_fourier_mfma<%s, list=%s, fused=%s>: %s' % (key + (r,)))
        assert r.get('ScratchSize', 0) == 0, (key, r)
        assert r.get('VGPRs', 0) + r.get('AGPRs', 0) <= 256, (key, r)
    assert any('3tcr20k_phase_factors_frag' in name for name in rows)


@pytest.fixture(scope='module')
def eng_gl(golden_env, built_lib):
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0).stage_env(golden_env)
    yield eng
    eng.close()


def _numpy_table(eng, phases):
    """gen_f as the reference spells it (track/bam_track.py:23-31), a block of storms at a time."""
    N, t = eng.n_series, np.asarray(eng.t_s, dtype=np.float64)
    T_Fs = eng.nl.T_days * 24 * 60 * 60
    nn = np.linspace(1, N, N)
    amp = np.sqrt(2 / np.sum(np.power(nn, -3)))
    wgt = np.power(nn, -1.5)[None, None, :, None]
    out = np.empty((phases.shape[0], 4, t.size))
    for a in range(0, phases.shape[0], 128):
        x = phases[a:a + 128, :, :, None]
        out[a:a + 128] = amp * np.sum(wgt * np.sin(2. * np.pi * (np.outer(nn, t)[None, None] / T_Fs + x)), axis=2)
    return out


@pytest.mark.gpu
def test_whole_table_bitwise(eng_gl):
    """engine.fourier_table: one storm, less than a row tile, more than one, and 4 x (workgroups along x) + 7 storms — some
    workgroups then walk to a second row tile and the last tile holds three storms.  Phases 0, 1/4, 1/2 and the largest
    double below 1 are planted in the first storm (sinpi / cospi at their exact zeros and at the end of the range)."""
    import torch
    eng = eng_gl
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wgs_x = 2 * cus                     # a one-piece table: two column groups along y share the chip's 4 x cus workgroups
    rng = np.random.default_rng(20)
    for n in (1, 2, 5, 4 * wgs_x + 7):
        ph = rng.uniform(0.0, 1.0, size=(n, 4, eng.n_series))
        for i, v in enumerate(PLANTED):
            ph[0, i, (3 * i) % eng.n_series] = v
            ph[n - 1, (i + 1) % 4, eng.n_series - 1 - i] = v
        try:
            eng.tune(table_factors=0)
            sep = eng.fourier_table(ph)
            eng.tune(table_factors=1)
            fused = eng.fourier_table(ph)
        finally:
            eng.tune(table_factors=-1)
        dflt = eng.fourier_table(ph)
        assert np.isfinite(sep).all()
        assert np.array_equal(sep.view(np.uint64), fused.view(np.uint64)), n
        assert np.array_equal(dflt.view(np.uint64), fused.view(np.uint64)), n
        err = np.abs(fused - _numpy_table(eng, ph)).max()
        print('fused table, n = %d: max |GPU - NumPy| = %.3g' % (n, err))
        assert err < 5e-14, (n, err)            # the bound of tests/test_gpu_parity.py::test_rhs_vs_reference_golden


@pytest.mark.gpu
@pytest.mark.parametrize('tc_rows_only', [False, True])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_two_segments_and_the_list_bitwise(eng_gl, dtype, tc_rows_only):
    """A chain over a segmented table: the second segment is written for the storms pass 0 parked, a count that is not a
    multiple of the row tile's four storms.  Every output of integrate is the fallback's."""
    eng = eng_gl
    got = {}
    try:
        eng.tune(waves=32, park=12, park_final=2)
        for knob in (0, 1):
            eng.tune(table_factors=knob)
            # (a pipeline of its own per run: the planes' NaN padding is remembered per pipeline.  Which storms the tail
            # compaction parks depends on the order the lanes pull from the queue, so pass 0's count varies by a few from run
            # to run — 2146 and 2151 here — and one run in four lands on a multiple of 4: such a run is drawn again, the
            # assertion below holds for the run that is compared)
            for attempt in range(5):
                got[knob] = (_seeded(eng, tc_rows_only, dtype, year=YEAR_ALL, n=B_ALL), eng.pass_stats())
                if got[knob][1][0]['parked'] % 4 != 0:
                    break
    finally:
        eng.tune(waves=-1, park=-1, park_final=-1, table_factors=-1)
    for knob in (0, 1):
        stats = got[knob][1]
        ran = [s for s in stats if s['requests'] > 0]
        print('table_factors = %d, %s, tc_rows_only = %s: parked per pass %s' % (knob, dtype, tc_rows_only, [s['parked'] for s in ran]))
        assert len(ran) >= 2, stats
        assert stats[0]['parked'] > 0 and stats[0]['parked'] % 4 != 0, stats
    sep, fused = got[0][0], got[1][0]
    assert sep['is_tc'].sum() >= 100 and (sep['n_valid'] > 192).sum() >= 1
    for k in COUNTERS:
        assert np.array_equal(sep[k], fused[k]), k
    for k in KEYS:
        assert np.array_equal(sep[k], fused[k], equal_nan=True), k
        view = np.uint64 if sep[k].dtype == np.float64 else np.uint32
        assert np.array_equal(sep[k].view(view), fused[k].view(view)), k


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [False, True])
def test_reset_by_the_table_kernel(golden_env, built_lib, graph):
    """flags[], the TC count and the queue words are now cleared by the fused table kernel: a round that follows a round
    with more TCs (other candidates) on the same pipeline gives what it gives on a fresh context — enqueued directly, and
    as the replay of a captured round."""
    from tropical_cyclone_risk_amd.engine import TCEngine
    keys = ((2003, 0), (2004, 7 * N_CAND))
    fresh = {}
    for key in keys:
        eng = TCEngine('GL', device=0).stage_env(golden_env)
        assert eng.tune()['table_factors'] != 0
        p = _pipe(eng, N_CAND, B, True)
        p.round(key[0], key[1], N_CAND, B)
        fresh[key] = p.host_tracks()
        eng.close()
    tcs = {key: int(fresh[key]['is_tc'].sum()) for key in keys}
    print('TCs per round:', tcs)
    assert min(tcs.values()) >= 100 and tcs[keys[0]] != tcs[keys[1]], tcs
    first, second = sorted(keys, key=lambda key: -tcs[key])       # the round with more TCs runs first
    eng = TCEngine('GL', device=0).stage_env(golden_env)
    p = _pipe(eng, N_CAND, B, True)
    for key in (first, first, second) if graph else (first, second):
        p.round(key[0], key[1], N_CAND, B, graph=graph)
    got, ref = p.host_tracks(), fresh[second]
    if graph:
        gs = p.graph_stats()
        assert gs['graphs'] == 1 and gs['replays'] >= 1, gs
    eng.close()
    for k in COUNTERS:
        assert np.array_equal(ref[k], got[k]), k
    assert np.array_equal(ref['is_tc'], got['is_tc'])
    for k in KEYS:
        assert np.array_equal(ref[k][ref['is_tc']], got[k][ref['is_tc']], equal_nan=True), k
