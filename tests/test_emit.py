"""The emission stage pinned at its own inputs: env winds, vmax and accept test 2 of k_emit / k_flags, fp32 and fp64.

tests/test_rk_steps.py, check 6, holds the emitted lon, lat, v, m and is_tc bit for bit.  Here the rest of what the same two kernels
write is recomputed on the CPU from the device's OWN emitted rows (tests/emit_numpy.py), so nothing is integrated on the reference
side and nothing is amplified:
  A  envw    equals the single-point probe at the row's own position, time, slot and forcing-table row, bit for bit;
  B  vmax    against oracle.scipy_port.max_wind on the rows, in units of emit_numpy.vmax_bound — a first-order forward error bound of
             vmax_at in the run's type, without a free constant; NaN exactly where n == 1 or i >= n;
  C  flags   is_tc and accepted equal emit_numpy.accept_flags on the device's v and vmax, and nothing but the two public bits is set;
  D  census  the batches hold storms that end at lane 0 and lane 63 of a wave and at both edges of a 128-thread workgroup, storms of
             one and of two samples, accepted and merely-is_tc storms, and both halves of fac.
The CPU tests prove the identity vmax = v + min(|U|, v / 2) the bound rests on, the bound itself (the device's formulation evaluated
with NumPy in float64 and float32 stays inside it on the golden rows), the checker (eight planted defects fail it) and the batches
(counted with the C oracle) before a GPU sees any of it.
"""
import os

import numpy as np
import pytest

from tests import emit_numpy as en
from tests import rk_steps_numpy as rk
from tests.test_rk_steps import BASIN, E_YEAR, N_CAND, _bits, _engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEYS = ('lon', 'lat', 'v0', 'm0', 'h_bl', 'month', 'phases')

# Candidates of E_YEAR appended to the first N_CAND, found with the C oracle on the CPU (test_batches_meet_their_conditions_by_the_oracle
# prints the census).  The first 256 hold 30 storms of one sample, 29 accepted storms, 2 storms with n % 64 == 63 and one with
# n % 64 == 0, but none with n % 64 == 1, none that is is_tc without being accepted and no storm of two samples: the first RK45 step
# is rarely shorter than two hours, and the oracle finds such a storm once in some 400 000 candidates — these four among the first
# 2.3 million (102383 has three samples in fp32, the other three have two in both types).  Of the other classes a few more than the
# oracle needs, since the fp32 run may give a storm another length or flip a flag.
EXTRA = dict(n2=(102383, 770167, 1959979, 2274973),
             w1=(810, 1009, 1995, 2082),                  # n_valid 193, 193, 129, 257
             w0=(1032, 1040),                             # 64, 320
             w63=(425, 568),                              # 319, 63
             tc_only=(1035, 2643, 2690, 3959, 4676, 7603, 8015, 11361, 11897, 12630, 12713, 17432))
EXTRA_CAND = tuple(sorted(c for v in EXTRA.values() for c in v))

# four short output grids at the default 3 600 s interval: a storm that reaches t_bound has n_valid = n_steps = 64, 65, 128, 129 —
# its last sample sits at lane 63 or lane 0 of a wave, or of a 128-thread workgroup
SHORT_DAYS = (63 / 24, 64 / 24, 127 / 24, 128 / 24)
SHORT_STEPS = (64, 65, 128, 129)
N_SHORT = 64

# B: the largest |vmax_dev - vmax_ref| / vmax_bound may be.  The next power of two at or above twice the maximum measured on the
# MI355X (MEASURED), at most 8; the planted defects are held to 8.
E_CAP = 8.0
E_BOUND = dict(f32=2.0, f64=1.0)
# max |vmax_dev - vmax_ref| / vmax_bound over all samples, the end samples, the wave-edge lanes (i % 64 in {0, 63}), the workgroup-edge
# threads (i % 128 in {0, 127}) and the two halves of fac; test_device_emission prints them
MEASURED = dict(f32=dict(all=0.832, end=0.375, wave=0.627, block=0.611, fac_lt1=0.384, fac_eq1=0.832),
                f64=dict(all=0.395, end=0.290, wave=0.360, block=0.283, fac_lt1=0.395, fac_eq1=0.084))


def _prm(total_time=None):
    from oracle.scipy_port import Params
    return Params() if total_time is None else Params(total_time=float(total_time))


def _total_time(days):
    return float(days * 24 * 60 * 60)                     # engine.params_from_namelist's expression


def _gather(seed_range, n_first, extra):
    parts = [seed_range(0, n_first)] + [seed_range(c, 1) for c in extra]
    return {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in KEYS}


def _oracle_seeder(env):
    from oracle import seeding
    from tropical_cyclone_risk_amd import namelist
    se = seeding.SeedEnv(env, BASIN)
    return lambda c0, n: seeding.seed_candidates(se, namelist.gpu_experiment_seed, E_YEAR, c0, n)


def _facs(out, dt_out):
    """per storm fac_of its rows, None for a storm without a vmax"""
    facs = []
    for i in range(len(out['n_valid'])):
        nv = int(out['n_valid'][i])
        if out['status'][i] == en.GATED or nv < 2:
            facs.append(None)
        else:
            facs.append(en.fac_of(out['lon'][i, :nv], out['lat'][i, :nv], out['v'][i, :nv], out['envw'][i, :nv], dt_out))
    return facs


def _check_census(batches, short_full):
    c = en.census(batches)
    print('census: ' + ', '.join('%s %d' % kv for kv in c.items()) + '; storms at t_bound on the short grids %s' % (short_full,))
    for k, need in en.CENSUS_MIN.items():
        assert c[k] >= need, (k, c[k], need)
    assert min(short_full) >= 3, short_full
    return c


# ------------------------------------------------------------------------------------------------ the golden rows
PREFIXES = (2, 3, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257)


def golden_rows(R):
    """Every golden NA / GL track of two samples or more as (lon, lat, v, envw, the file's vmax), float64 — rounded to R first — and
    its first 2, 3, 63, ... 257 rows as tracks of their own (file's vmax: None), which end at every lane the kernel treats apart."""
    rows = []
    for basin in ('NA', 'GL'):
        g = np.load(os.path.join(GOLDEN, 'tracks_%s.npz' % basin))
        for k in range(len(g['n_valid'])):
            n = int(g['n_valid'][k])
            if n < 2:
                continue
            full = tuple(a.astype(R).astype(np.float64) for a in (g['traj'][k, 0, :n], g['traj'][k, 1, :n], g['traj'][k, 2, :n], g['envw'][k, :n]))
            rows.append(full + (g['vmax'][k, :n],))
            rows += [tuple(a[:p] for a in full) + (None,) for p in PREFIXES if p < n]
    return rows


def _max_error(R, rows, dt_out, **plant):
    """(the largest normalised error of vmax_in over the rows, the number of samples above E_CAP)"""
    worst, over = 0.0, 0
    for lon, lat, v, w, _ in rows:
        e = en.vmax_errors(R, en.vmax_in(R, lon, lat, v, w, dt_out, **plant), lon, lat, v, w, dt_out)
        assert not np.isnan(e).any()
        worst, over = max(worst, float(e.max())), over + int((e > E_CAP).sum())
    return worst, over


# ------------------------------------------------------------------------------------------------ CPU tests
def test_vmax_identity_and_golden_vmax():
    """vmax = v + min(|U|, v / 2) (emit_numpy.vmax_identity), on which vmax_bound rests, against max_wind on every golden row: to
    1e-12; and max_wind reproduces the files' own vmax to the 1e-12 of tests/test_oracle_golden.py."""
    dt_out = _prm().dt_out
    worst = own = 0.0
    n = 0
    for lon, lat, v, w, vm in golden_rows(np.float64):
        ref = en.vmax_ref(lon, lat, v, w, dt_out)
        worst = max(worst, float(np.abs(en.vmax_identity(lon, lat, v, w, dt_out) - ref).max()))
        if vm is not None:
            own = max(own, float(np.abs(ref - vm).max()))
            n += len(vm)
    print('identity within %.2g of max_wind; the files\' vmax within %.2g on %d samples' % (worst, own, n))
    assert worst <= 1e-12 and own <= 1e-12 and n > 5000


@pytest.mark.parametrize('R', [np.float64, np.float32])
def test_device_formulation_within_the_bound(R):
    """vmax_in(R) — the device's formulation in NumPy — against max_wind on the golden rows rounded to R: every sample's
    |a - b| / vmax_bound(R) <= 1.  Found: 0.50 in float64, on a sample with fac < 1, where both sides round 1.5 v their own way
    (0.035 where fac == 1: the reference converts to radians first as well, so the dominant rounding is common to both); 0.73 in
    float32, where it is not common: the bound is within a factor 1.4 of what happens."""
    rows = golden_rows(R)
    worst, _ = _max_error(R, rows, _prm().dt_out)
    print('%s: %d tracks, %d samples, max normalised error %.3f' % (R.__name__, len(rows), sum(len(r[0]) for r in rows), worst))
    assert worst <= 1.0


@pytest.mark.parametrize('R', [np.float64, np.float32])
def test_planted_defects_fail_the_checker(R):
    """Each defect of emit_numpy.DEFECTS planted in vmax_in must push a sample's normalised error above 8 on the golden rows.  The
    relative perturbation of vmax starts at 2^-14 (float32) / 2^-44 (float64) and is doubled until it is seen; none above 2^-11 /
    2^-40 may go unseen.  Needed: 2^-14 / 2^-44, where 22 606 / 21 202 of the 47 379 samples fail."""
    rows = golden_rows(R)
    dt_out = _prm().dt_out
    for d in en.DEFECTS[:-1]:
        worst, over = _max_error(R, rows, dt_out, defect=d)
        print('%s %-17s max normalised error %.3g, %d samples above %g' % (R.__name__, d, worst, over, E_CAP))
        assert over > 0, d
    first, last = (14, 11) if R == np.float32 else (44, 40)
    for k in range(first, last - 1, -1):
        worst, over = _max_error(R, rows, dt_out, defect='relative', rel=2.0 ** -k)
        print('%s relative 2^-%d: max normalised error %.3g, %d samples above %g' % (R.__name__, k, worst, over, E_CAP))
        if over:
            break
    assert over > 0, 'a relative defect of 2^-%d goes unseen: the bound is too loose' % last


def test_accept_flags_on_the_golden_tracks():
    """emit_numpy.accept_flags on the golden NA / GL rows gives the files' is_tc and accepted (both values of each occur)."""
    prm = _prm()
    grid = rk.Grid(prm.total_time, prm.n_steps)
    seen = set()
    for basin in ('NA', 'GL'):
        g = np.load(os.path.join(GOLDEN, 'tracks_%s.npz' % basin))
        for k in range(len(g['n_valid'])):
            got = en.accept_flags(np.float64, g['traj'][k, 2], g['vmax'][k], g['n_valid'][k], g['status'][k], grid,
                                  prm.v_thresh, prm.v_2d_thresh, prm.vmax_thresh)
            assert got == (bool(g['is_tc'][k]), bool(g['accepted'][k])), (basin, k)
            seen.add(got)
    assert (True, True) in seen and (False, False) in seen


def test_batches_meet_their_conditions_by_the_oracle(golden_env):
    """What test_device_emission needs of its batches, counted with the C oracle alone (the oracle's seeding is the device's,
    tests/test_seeding.py): emit_numpy.CENSUS_MIN over the main batch — the first 256 GL candidates of E_YEAR and EXTRA_CAND — and
    the four short grids of 64 candidates, and on each short grid at least 3 storms that reach t_bound.  Counted: see the print."""
    from oracle import c_oracle
    seeder = _oracle_seeder(golden_env)
    main = _gather(seeder, N_CAND, EXTRA_CAND)
    batches, short_full = [], []

    def run(storms, prm):
        ref = c_oracle.run_ensemble(golden_env, BASIN, storms, prm=prm)
        ref.update(lon=ref['traj'][:, 0], lat=ref['traj'][:, 1], v=ref['traj'][:, 2])
        ref['fac'] = _facs(ref, prm.dt_out)
        return ref
    ref = run(main, _prm())
    batches.append(ref)
    nv = ref['n_valid'][N_CAND:]
    print('extra candidates %s: n_valid %s' % (EXTRA_CAND, list(nv)))
    short = {k: v[:N_SHORT] for k, v in main.items()}
    for days, steps in zip(SHORT_DAYS, SHORT_STEPS):
        prm = _prm(_total_time(days))
        assert prm.n_steps == steps
        r = run(short, prm)
        batches.append(r)
        short_full.append(int(((r['status'] != en.GATED) & (r['n_valid'] == steps)).sum()))
    _check_census(batches, short_full)


# ------------------------------------------------------------------------------------------------ GPU test
@pytest.fixture(scope='module')
def emit_engines(golden_env, built_lib):
    """the default engine and the four short-grid engines, staged once for both types"""
    from tests.test_gpu_parity import _namelist_with
    from tropical_cyclone_risk_amd.engine import TCEngine
    engines = [_engine(golden_env)]
    try:
        for days in SHORT_DAYS:
            engines.append(TCEngine(BASIN, device=0, nl=_namelist_with(total_track_time_days=days)).stage_env(golden_env))
        yield engines
    finally:
        for e in engines:
            e.close()


def check_emission(eng, storms, dtype, tot):
    """A, B, C on one batch; adds to the totals `tot` and returns what the census needs."""
    from tropical_cyclone_risk_amd import _lib
    R = np.float32 if dtype == 'f32' else np.float64
    P = eng.params
    dt_out = float(P.dt_out)
    grid = rk.Grid(float(P.total_time), eng.n_steps)
    out = eng.integrate(storms, dtype=dtype)
    assert out['vmax'].dtype == R and out['envw'].dtype == R
    assert ((out['flags'] & ~np.int32(_lib.FLAG_IS_TC | _lib.FLAG_ACCEPTED)) == 0).all()
    assert (_lib.FLAG_IS_TC | _lib.FLAG_ACCEPTED) < (1 << 8)
    Fs = eng.fourier_table(storms['phases'])
    for i in range(len(out['status'])):
        nv = int(out['n_valid'][i])
        assert np.isnan(out['vmax'][i, nv:]).all() and np.isnan(out['envw'][i, nv:]).all(), i
        flags = en.accept_flags(R, out['v'][i], out['vmax'][i], nv, out['status'][i], grid, float(P.v_thresh), float(P.v_2d_thresh), float(P.vmax_thresh))
        assert flags == (bool(out['is_tc'][i]), bool(out['accepted'][i])), (i, flags)                                    # C
        if out['status'][i] == en.GATED:
            assert nv == 0, i
            continue
        lon, lat, v, m = (out[k][i, :nv].astype(np.float64) for k in ('lon', 'lat', 'v', 'm'))
        w = eng.probe_rhs(int(storms['month'][i]) - 1, float(storms['h_bl'][i]), Fs[i], eng.t_s[:nv], lon, lat, v, m, dtype=dtype)[1]      # A
        assert np.array_equal(w.astype(R).astype(np.float64), w, equal_nan=True), i
        tot['envw_bad'] += int((_bits(w.astype(R)) != _bits(out['envw'][i, :nv])).any(axis=1).sum())
        tot['rows'] += nv
        tot['storms'] += 1
        vm = out['vmax'][i, :nv]                                                                                           # B
        if nv == 1:
            assert np.isnan(vm[0]), i
            continue
        assert not np.isnan(vm).any(), i
        envw = out['envw'][i, :nv].astype(np.float64)
        e = en.vmax_errors(R, vm, lon, lat, v, envw, dt_out)
        assert not np.isnan(e).any(), i
        tot['abs'] = max(tot.get('abs', 0.0), float(np.abs(vm.astype(np.float64) - en.vmax_ref(lon, lat, v, envw, dt_out)).max()))
        fac = en.fac_of(lon, lat, v, envw, dt_out)
        masks = dict(en.sample_classes(nv), all=np.ones(nv, bool), fac_lt1=fac < 1, fac_eq1=fac == 1)
        for k, mk in masks.items():
            if mk.any():
                tot['e_' + k] = max(tot.get('e_' + k, 0.0), float(e[mk].max()))
        tot['vmax_samples'] += nv
    out['fac'] = _facs(out, dt_out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_device_emission(golden_env, emit_engines, dtype):
    """A to D of the module docstring on what k_emit<float> / <double> and k_flags write, all rows (eng.integrate): the main batch —
    the first 256 GL candidates of E_YEAR and EXTRA_CAND as eng.seed gives them, 361 samples: workgroup edges at 127 / 128 and
    255 / 256, wave edges every 64 — and 64 candidates on each of four short grids of 64, 65, 128 and 129 samples.  The batches were
    counted on the CPU first (test_batches_meet_their_conditions_by_the_oracle); D counts them again on the device's own n_valid and
    flags.
    Measured on the MI355X (MEASURED), fp32 / fp64: 342 integrated storms, 40 775 / 40 785 rows;
      A  0 env-wind rows differ from the probe;
      B  40 713 / 40 723 samples; max normalised error 0.832 / 0.395 (E_BOUND 2 / 1); ends 0.375 / 0.290, wave-edge lanes 0.627 / 0.360,
         workgroup-edge threads 0.611 / 0.283, fac < 1 0.384 / 0.395, fac == 1 0.832 / 0.084.  In fp32 the largest errors are the
         radians-first cancellation of the fac == 1 half, which the float64 reference does not share; in fp64 it does, and what is
         left is the rounding of 1.5 v where fac < 1;
      C  every is_tc and accepted as restated, no other bit set;
      D  n_valid == 1: 62, == 2: 3 / 4, % 64 == 0: 47, == 1: 48, == 63: 4, % 128 in {0, 1}: 37; 53 accepted, 12 is_tc only;
         24 404 / 24 415 samples with fac < 1, 16 309 / 16 308 with fac == 1; 27, 27, 17, 17 storms at t_bound on the short grids."""
    eng = emit_engines[0]
    main = _gather(lambda c0, n: eng.seed(E_YEAR, c0, n), N_CAND, EXTRA_CAND)
    short = {k: v[:N_SHORT] for k, v in main.items()}
    tot = dict(envw_bad=0, rows=0, storms=0, vmax_samples=0)
    batches = [check_emission(eng, main, dtype, tot)]
    short_full = []
    for e, steps in zip(emit_engines[1:], SHORT_STEPS):
        assert e.n_steps == steps
        out = check_emission(e, short, dtype, tot)
        batches.append(out)
        short_full.append(int(((out['status'] != en.GATED) & (out['n_valid'] == steps)).sum()))
    print('%s: %d integrated storms, %d rows; A: %d env-wind rows differ from the probe' % (dtype, tot['storms'], tot['rows'], tot['envw_bad']))
    print('%s: B: %d samples; max normalised vmax error %.4f; ends %.4f, wave edges %.4f, workgroup edges %.4f, fac < 1 %.4f, fac == 1 %.4f (bound %g); '
          'max |vmax_dev - vmax_ref| %.3g m/s'
          % (dtype, tot['vmax_samples'], tot['e_all'], tot['e_end'], tot['e_wave'], tot['e_block'], tot['e_fac_lt1'], tot['e_fac_eq1'], E_BOUND[dtype], tot['abs']))
    _check_census(batches, short_full)                                                                                     # D
    assert tot['envw_bad'] == 0 and tot['rows'] > 20000
    assert E_BOUND[dtype] <= E_CAP and tot['e_all'] <= E_BOUND[dtype]
