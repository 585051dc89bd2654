"""Accept test 1 decided inside the integrator (TC-rows-only mode, KArgsT::tc_list).

With tcr_tracks.tc_rows_only, tcr_tune.prune != 0 and 2 d an output sample, k_integrate judges `any(v >= 15) and
v(2 d) >= 6.5` (util/compute.py:185-189) on every step it accepts and appends the storms that pass to the TC list;
k_screen is not launched and the v part of the step records is not written.  The fallback (prune = 0, or 2 d between two
samples) is k_screen over every storm.  Both take the decision on the same v, formed by the same helpers
(tcr_device.h: dense_v_*), so everything here is compared with np.array_equal: counters and flags of every storm, rows of
is_tc storms bit for bit, rows of the others untouched (the planes are pre-filled).
"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ('lon', 'lat', 'v', 'm', 'vmax', 'envw')
COUNTERS = ('n_valid', 'status', 'flags', 'nfev', 'n_accept', 'n_reject')
FILL = 123.0
YEAR, B, N_CAND = 2005, 4096, 40_000
# The batch of the first test: the first 8192 passing seeds of GL, 2012.  Counted with the CPU oracles (oracle/seeding.py +
# oracle/c_oracle.py) before anything ran on a GPU: 466 TCs, 1849 tracks that end before 2 d below 6.5 m/s and ONE at or above it
# (storm 4906: 44 samples, v(last) = 8.61 — a track that leaves through the equator band; 2 such storms in 16 years x 8192),
# 51 maxima in [14, 15) and 53 in [15, 16].  No year of 2001-2016 has all the classes within its first 4096 storms.
YEAR_ALL, B_ALL = 2012, 8192


def _namelist_with(**over):
    from tropical_cyclone_risk_amd import namelist
    nl = types.SimpleNamespace(**{k: getattr(namelist, k) for k in dir(namelist) if not k.startswith('__')})
    for k, v in over.items():
        setattr(nl, k, v)
    return nl


def _pipe(eng, n_cand, n, tc_rows_only, dtype='f64'):
    from tropical_cyclone_risk_amd.pipeline import DevicePipeline
    p = DevicePipeline(eng, n_cand, n, tc_rows_only=tc_rows_only, dtype=dtype)
    for k in KEYS:
        p.tracks[k].fill_(FILL)
    return p


def _seeded(eng, tc_rows_only, dtype='f64', year=YEAR, n=B, n_cand=N_CAND):
    p = _pipe(eng, n_cand, n, tc_rows_only, dtype)
    p.seed_round(year, 0); p.select_passed(n)
    assert int(p.n_passed.item()) >= n
    p.integrate(n)
    return p.host_tracks()


def _same_decision(full, tc, tag, counters=COUNTERS):
    """tc (TC rows only, planes pre-filled) against full (all rows): counters and flags of every storm, rows of is_tc
    storms, and the other rows still hold the fill."""
    for k in counters:
        assert np.array_equal(full[k], tc[k]), (tag, k)
    is_tc = full['is_tc']
    for k in KEYS:
        assert np.array_equal(full[k][is_tc], tc[k][is_tc], equal_nan=True), (tag, k)
        assert (tc[k][~is_tc] == FILL).all(), (tag, k)


def _classes(full, sample_2d, v_2d=6.5):
    """The cases the in-flight decision distinguishes, counted on the all-rows result."""
    n, v = full['n_valid'], full['v'].astype(np.float64)
    alive = n > 0
    short = alive & (n - 1 < sample_2d)                       # the track ends before the 2-day sample
    v_last = v[np.arange(len(n)), np.clip(n - 1, 0, None)]
    with np.errstate(invalid='ignore'):
        vmax = np.where(alive, np.nanmax(np.where(np.isnan(v), -np.inf, v), axis=1), np.nan)
    return dict(tcs=int(full['is_tc'].sum()),
                short_pass=int((short & (v_last >= v_2d)).sum()), short_fail=int((short & (v_last < v_2d)).sum()),
                below15=int(((vmax >= 14.0) & (vmax < 15.0)).sum()), above15=int(((vmax >= 15.0) & (vmax <= 16.0)).sum()))


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_in_flight_equals_k_screen_and_all_rows(golden_env, built_lib, dtype):
    """Default tune (in flight) == prune = 0 (k_screen over every storm) == all rows, on a batch that holds every case:
    tracks that end before 2 d on either side of 6.5 m/s, and maxima just below and just above 15 m/s."""
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0).stage_env(golden_env)
    full = _seeded(eng, False, dtype, year=YEAR_ALL, n=B_ALL)
    cls = _classes(full, 48)
    print('in-flight accept test, %s, year %d, %d storms: %s' % (dtype, YEAR_ALL, B_ALL, cls))
    assert cls['tcs'] >= 100 and cls['short_pass'] >= 1 and cls['short_fail'] >= 1, cls
    assert cls['below15'] >= 1 and cls['above15'] >= 1, cls
    inflight = _seeded(eng, True, dtype, year=YEAR_ALL, n=B_ALL)
    eng.tune(prune=0)
    try:
        fallback = _seeded(eng, True, dtype, year=YEAR_ALL, n=B_ALL)
    finally:
        eng.tune(prune=-1)
    eng.close()
    _same_decision(full, inflight, (dtype, 'in flight'))
    _same_decision(full, fallback, (dtype, 'k_screen'))
    for k in COUNTERS:
        assert np.array_equal(inflight[k], fallback[k]), (dtype, k)
    for k in KEYS:
        assert np.array_equal(inflight[k], fallback[k], equal_nan=True), (dtype, k)


def test_state_survives_parking(golden_env, built_lib):
    """The per-storm state of the test (any15, the 2-day state) travels in the park record: a chain of at least three passes
    over a segmented forcing table gives what one pass gives."""
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0).stage_env(golden_env)
    eng.tune(park=0)
    try:
        one_pass = _seeded(eng, True)
        eng.tune(waves=32, park=12, park_final=2)
        chained = _seeded(eng, True)
        stats = eng.pass_stats()
    finally:
        eng.tune(waves=-1, park=-1, park_final=-1)
    eng.close()
    ran = [s for s in stats if s['requests'] > 0]
    assert len(ran) >= 3 and sum(s['parked'] for s in stats) > 0, stats
    # a TC that lives beyond the first table segment (192 samples) was parked at the boundary and restored
    assert (chained['n_valid'][chained['is_tc']] > 192).sum() >= 1
    assert chained['is_tc'].sum() >= 100
    for k in COUNTERS:
        assert np.array_equal(one_pass[k], chained[k]), k
    for k in KEYS:
        assert np.array_equal(one_pass[k], chained[k], equal_nan=True), k


@pytest.mark.parametrize('dt_out,days,T_days', [(5400, 10, 20), (1800, 9, 20), (3600, 15, 17.3), (7000, 15, 20)])
def test_output_grids(golden_env, built_lib, dt_out, days, T_days):
    """2 d is output sample 32 / 96 / 48 (in flight) or lies between two samples (7000 s: k_screen): the same as all rows."""
    from tropical_cyclone_risk_amd import synthetic
    from tropical_cyclone_risk_amd.engine import TCEngine
    n = 2048
    nl = _namelist_with(output_interval_s=dt_out, total_track_time_days=days, T_days=T_days)
    storms = synthetic.draw_storm_inputs(n, 'NA', seed=5 + dt_out)
    eng = TCEngine('NA', device=0, nl=nl).stage_env(golden_env)
    out = []
    for tc_rows_only in (False, True):
        p = _pipe(eng, 64, n, tc_rows_only)
        p.load_storms(storms)
        p.integrate(n)
        out.append(p.host_tracks())
    eng.close()
    full, tc = out
    print('output grid %d s x %d d: %d TCs of %d storms' % (dt_out, days, full['is_tc'].sum(), n))
    assert full['is_tc'].sum() >= 1 and (~full['is_tc']).sum() >= 1
    _same_decision(full, tc, dt_out)


def test_short_step_records(golden_env, built_lib):
    """Steps beyond the record's capacity are not looked at by either path: with room for 8 accepted steps per storm the
    in-flight flags are k_screen's for every storm, overflowed ones included."""
    from tropical_cyclone_risk_amd import _lib
    from tropical_cyclone_risk_amd.engine import TCEngine
    n = 2048
    eng = TCEngine('GL', device=0, nl=_namelist_with(gpu_max_rk_steps=8)).stage_env(golden_env)
    inflight = _seeded(eng, True, n=n, n_cand=20_000)
    eng.tune(prune=0)
    try:
        fallback = _seeded(eng, True, n=n, n_cand=20_000)
    finally:
        eng.tune(prune=-1)
    eng.close()
    assert (inflight['status'] == _lib.STATUS_STEP_OVERFLOW).sum() >= 1
    assert (fallback['status'] == _lib.STATUS_STEP_OVERFLOW).sum() >= 1
    assert np.array_equal(inflight['flags'], fallback['flags'])


def test_replayed_round(golden_env, built_lib):
    """The TC list's count and flags[] are reset inside the captured round: replays with other candidates give the flags
    and the TC rows of the same rounds enqueued directly."""
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0).stage_env(golden_env)
    direct, replayed = _pipe(eng, N_CAND, B, True), _pipe(eng, N_CAND, B, True)
    for year, cand0 in ((2003, 0), (2003, N_CAND), (2004, 7 * N_CAND)):
        direct.round(year, cand0, N_CAND, B)
        replayed.round(year, cand0, N_CAND, B, graph=True)
        a, b = direct.host_tracks(), replayed.host_tracks()
        assert a['is_tc'].sum() >= 100
        assert np.array_equal(a['flags'], b['flags']), (year, cand0)
        for k in KEYS:
            assert np.array_equal(a[k][a['is_tc']], b[k][a['is_tc']], equal_nan=True), (year, cand0, k)
    gs = replayed.graph_stats()
    assert gs['graphs'] == 1 and gs['replays'] >= 2, gs
    eng.close()
