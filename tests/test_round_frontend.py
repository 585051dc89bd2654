"""The front end of tcr_round_dev — seeding, selection of the seeds that pass, locality order, gather of the dense batch and its
phases — against the staged entry points it must reproduce bit for bit (tcr_seed_dev, tcr_compact_dev, tcr_cell_order_dev,
tcr_gather_seeds_dev, tcr_integrate[_f32]_dev), at the small shapes where a selection can go wrong; tests/test_round.py
compares whole rounds at 24 000 candidates.

Shapes: a selection tile is kScanTile = kScanThreads * kScanItems = 2 048 candidates (tcr_compact.hip), so N_CAND = 3 * 2048 +
101 is three full tiles and a partial one: every tile but the first looks back over published counts, the last one is cut by
n_cand.  Between 1 % and 48 % of the candidates pass (asserted below), so B_BELOW clips the selection and B_ABOVE does not."""
import re
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEL_TILE = 2048
N_CAND = 3 * SEL_TILE + 101
B_BELOW, B_ABOVE = 60, 3000
SEED_KEYS = ('lon0', 'lat0', 'v0', 'm0', 'h_bl', 'slot', 'basin_idx', 'seed_flags')
TRACK_KEYS = ('n_valid', 'status', 'flags', 'nfev', 'n_accept', 'n_reject', 'lon', 'lat', 'v', 'm')


def test_the_tile_size_is_the_one_in_the_source():
    src = open(os.path.join(os.path.dirname(__file__), '..', 'tropical_cyclone_risk_amd', 'csrc', 'tcr_compact.hip')).read()
    threads = int(re.search(r'constexpr int kScanThreads = (\d+);', src).group(1))
    items = int(re.search(r'constexpr int kScanItems = (\d+);', src).group(1))
    assert threads * items == SEL_TILE


def _pipeline(eng, B, order, dtype='f64'):
    """A pipeline whose outputs start from a sentinel, so that rows no path may write compare equal too."""
    from tropical_cyclone_risk_amd.pipeline import DevicePipeline
    p = DevicePipeline(eng, N_CAND, B, sort_storms=order, dtype=dtype)
    for d in (p.cand, p.storms):
        for k, v in d.items():
            if k != 'n' and v is not None:
                v.fill_(-3)
    for v in p.tracks.values():
        v.fill_(-3)
    p.cand_idx.fill_(-3)
    return p


def _staged(p, year, cand0, B, exact):
    p.seed_round(year, cand0, N_CAND)
    p.select_passed(B)
    p.integrate(B, n_dev=p.n_passed if exact else None)


def _round(p, year, cand0, B, exact, graph=False):
    p.round(year, cand0, N_CAND, B, exact_count=exact, graph=graph)


def _snap(p, B):
    """Device copies (stream ordered: no host synchronisation between two rounds)."""
    s = {'n_passed': p.n_passed.clone(), 'cand_idx': p.cand_idx[:B].clone()}
    s.update({'storms.' + k: p.storms[k][:B].clone() for k in SEED_KEYS + ('phases',)})
    s.update({'cand.' + k: p.cand[k][:N_CAND].clone() for k in SEED_KEYS})
    s.update({'tracks.' + k: p.tracks[k][:B].clone() for k in TRACK_KEYS})
    return s


def _same(a, b, what, B, exact=True):
    n_pass = int(a['n_passed'].item())
    assert n_pass == int(b['n_passed'].item()), what
    rows = min(n_pass, B) if exact else B
    for k in a:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        if k.startswith('tracks.'):
            x, y = x[:rows], y[:rows]              # (rows that hold no storm are not integrated)
        assert np.array_equal(x, y, equal_nan=True), (what, k, int((x != y).sum()))
    return n_pass


@pytest.mark.parametrize('basin,order,B,exact', [
    ('GL', 2.0, B_ABOVE, True),        # 16 380 cells: keys and cell counts come out of the compaction
    ('GL', 2.0, B_BELOW, False),       # ... clipped at n_storms; n_passed stays the total
    ('AU', 30.0, B_ABOVE, True),       # 84 cells: the few-cell path (counts in LDS, k_cell_key in a launch of its own)
    ('AU', 30.0, B_BELOW, False),
    ('GL', False, B_BELOW, True),      # no order: dense row = rank
    ('GL', False, B_ABOVE, True),
])
def test_round_equals_the_staged_calls(golden_env, built_lib, basin, order, B, exact):
    import torch
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine(basin, device=0).stage_env(golden_env)
    ref, one = _pipeline(eng, B, order), _pipeline(eng, B, order)
    _staged(ref, 2003, 5 * N_CAND, B, exact)
    _round(one, 2003, 5 * N_CAND, B, exact)
    torch.cuda.synchronize()
    n_pass = _same(_snap(ref, B), _snap(one, B), (basin, order, B, exact), B, exact)
    assert (B_BELOW < n_pass < B_ABOVE), n_pass      # the two capacities are what their names say
    k = min(n_pass, B)
    ci = one.cand_idx[:k].cpu().numpy()
    assert len(np.unique(ci)) == k and (one.cand['seed_flags'].cpu().numpy()[ci] & 2).all()
    if not order:
        assert (np.diff(ci) > 0).all()
    assert (one.cand_idx[k:B] == -3).all() and (one.storms['lon0'][k:B] == -3).all()
    eng.close()


def test_four_rounds_back_to_back_reuse_the_scratch(golden_env, built_lib):
    """The ticket and generation words are left ready by one launch for the next: no host sync in between."""
    import torch
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0).stage_env(golden_env)
    ref, one = _pipeline(eng, B_ABOVE, 2.0), _pipeline(eng, B_ABOVE, 2.0)
    keys = [(2001, 0), (2001, N_CAND), (2010, 7 * N_CAND + 3), (1995, 10**6)]
    got = []
    for year, cand0 in keys:
        _round(one, year, cand0, B_ABOVE, True)
        got.append(_snap(one, B_ABOVE))
    want = []
    for year, cand0 in keys:
        _staged(ref, year, cand0, B_ABOVE, True)
        want.append(_snap(ref, B_ABOVE))
    torch.cuda.synchronize()
    for key, a, b in zip(keys, want, got):
        _same(a, b, key, B_ABOVE)
    assert len({int(b['n_passed'].item()) for b in got}) > 1          # the rounds differ
    eng.close()


def test_a_captured_round_replays_with_other_keys(golden_env, built_lib):
    """RoundKey: the replayed seeding and the phase draw read seed / year / cand0 on the device."""
    import torch
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0).stage_env(golden_env)
    ref, one = _pipeline(eng, B_ABOVE, 2.0), _pipeline(eng, B_ABOVE, 2.0)
    for year, cand0 in ((2001, 0), (2007, 2**32 + 12345), (1999, 3 * N_CAND)):
        _staged(ref, year, cand0, B_ABOVE, True)
        _round(one, year, cand0, B_ABOVE, True, graph=True)
        torch.cuda.synchronize()
        _same(_snap(ref, B_ABOVE), _snap(one, B_ABOVE), (year, cand0), B_ABOVE)
    gs = one.graph_stats()
    assert gs['graphs'] == 1 and gs['replays'] == 2, gs
    eng.close()


def test_two_contexts_on_two_streams(golden_env, built_lib):
    """The scratch is per context: rounds of two contexts interleaved on two streams do not meet."""
    import torch
    from tropical_cyclone_risk_amd.engine import TCEngine
    engs = [TCEngine('GL', device=0).stage_env(golden_env) for _ in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=0) for _ in range(2)]
    keys = [[(2001, 0), (2002, N_CAND)], [(2011, 4 * N_CAND), (2012, 9 * N_CAND)]]
    ones = [_pipeline(e, B_ABOVE, 2.0) for e in engs]
    torch.cuda.synchronize()
    got = [[], []]
    for it in range(2):
        for j in range(2):
            with torch.cuda.stream(streams[j]):
                _round(ones[j], *keys[j][it], B_ABOVE, True)
                got[j].append(_snap(ones[j], B_ABOVE))
    torch.cuda.synchronize()
    for j in range(2):
        ref = _pipeline(engs[j], B_ABOVE, 2.0)
        for it in range(2):
            _staged(ref, *keys[j][it], B_ABOVE, True)
            torch.cuda.synchronize()
            _same(_snap(ref, B_ABOVE), got[j][it], (j, it), B_ABOVE)
    for e in engs:
        e.close()


def test_round_with_the_phase_factors_in_a_kernel_of_their_own(golden_env, built_lib):
    """tcr_tune.table_factors = 0: the table kernels read the fragments k_phase_factors_frag forms from the gathered phases."""
    import torch
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0).stage_env(golden_env)
    assert eng.tune(table_factors=0)['table_factors'] == 0
    ref, one = _pipeline(eng, B_ABOVE, 2.0), _pipeline(eng, B_ABOVE, 2.0)
    _staged(ref, 2004, 2 * N_CAND, B_ABOVE, True)
    _round(one, 2004, 2 * N_CAND, B_ABOVE, True)
    torch.cuda.synchronize()
    _same(_snap(ref, B_ABOVE), _snap(one, B_ABOVE), 'table_factors=0', B_ABOVE)
    eng.close()


def test_round_f32(golden_env, built_lib):
    """The front end is fp64 in both modes; the fp32 path gets the same phases and gives the staged fp32 tracks."""
    import torch
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0).stage_env(golden_env)
    ref, one = _pipeline(eng, B_ABOVE, 2.0, 'f32'), _pipeline(eng, B_ABOVE, 2.0, 'f32')
    _staged(ref, 2004, 2 * N_CAND, B_ABOVE, True)
    _round(one, 2004, 2 * N_CAND, B_ABOVE, True)
    torch.cuda.synchronize()
    _same(_snap(ref, B_ABOVE), _snap(one, B_ABOVE), 'f32', B_ABOVE)
    eng.close()
