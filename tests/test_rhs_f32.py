"""The fp32 right-hand side pinned pointwise (tcr_probe_rhs_f32_host, tcr_probe_math_host fn 6-12).

Whole fp32 tracks (tcr_integrate_f32_*, DevicePipeline(dtype='f32'), BASELINE config 5) are held by distribution statistics of
ensembles, the RK45 step by its records (tests/test_rk_steps.py); here the function it integrates: nothing is integrated (except part E's tie to the shipped kernels), so nothing is amplified:
  A  the 20 lookups of an evaluation, bit for bit against tests/rhs_f32_numpy.py (NumPy float32, no fused operation), on every
     static storage mode, on affine and general axes, at the clamps, the end knots, one ulp around knots, in all-land / all-sea cells;
  B  the discrete branches give the oracle's branch and the exact constants;
  C  the continuous outputs against the fp64 C oracle on the same float-rounded data, in units of the oracle's own response to one
     float32 ulp of the inputs plus 2^-24 of the outputs' additive terms;
  D  the float helpers (division, square roots: IEEE bit for bit; pow, cos, exp: libm class);
  E  the probe's env winds equal the rows k_emit<float> writes, bit for bit, and the ventilation gate of k_integrate<float>
     agrees with its float32 restatement.
The CPU tests prove the restatement (its float64 mode equals the C oracle's bilinear bit for bit) and the checker of part C
(planted defects of 2^-14 fail, the undisturbed oracle passes) before a GPU sees either.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import rhs_f32_numpy as rn

SLOT = 8
H_BL = 1400.0

# Part C: bound on the normalised error |fp32 - oracle| / (twin + 2^-24 mag) per output = 4 x the maximum measured on the MI355X
# over both basins, rounded up to one digit (test_continuous_rhs_against_oracle states the measured maxima).
C_MEASURED = dict(dlon=5.30, dlat=1.95, dv=1.65, dm=1.76, envw0=1.96, envw1=2.15, envw2=2.73, envw3=2.22, alpha=1.16)
C_BOUNDS = dict(dlon=30.0, dlat=8.0, dv=7.0, dm=8.0, envw0=8.0, envw1=9.0, envw2=20.0, envw3=9.0, alpha=5.0)
PLANT = 2.0 ** -14


def _phases():
    return np.random.default_rng(41).uniform(0, 1, (4, 15))


@pytest.fixture(scope='module')
def envs(golden_env):
    """The environments of part A by name (built on first use, shared)."""
    from tropical_cyclone_risk_amd import synthetic
    cache = {}

    def get(name):
        if name not in cache:
            if name == 'golden':
                e = golden_env
            elif name in ('gfdl', 'gaussian'):
                e = synthetic.make_env(name, seed=7)
            elif name in ('i16', 'f32', 'f64'):                      # the reference's 0.125-degree int8 land + that bathymetry
                e = synthetic.make_env('era5', static_res=0.125, bathy_kind=name)
            elif name == 'two_grids':                                # land at 0.125 degrees, float32 bathymetry on its own 0.25-degree grid
                e8, e4 = get('f32'), synthetic.make_env('era5', static_res=0.25, bathy_kind='f32')
                e = dataclasses.replace(e8, bathy=e4.bathy, blon=e4.hlon, blat=e4.hlat)
            else:
                raise KeyError(name)
            cache[name] = e
        return cache[name]
    return get


# (environment, basin, gpu_static_store, static mode the context ends in)
CASES = [('golden', 'GL', 'auto', 'f64'), ('golden', 'NA', 'auto', 'f64'),
         ('gfdl', 'WP', 'auto', 'f64'), ('gaussian', 'EP', 'auto', 'f64'),
         ('i16', 'NA', 'auto', 'pack16'), ('f32', 'NA', 'auto', 'pack64'), ('two_grids', 'NA', 'auto', 'u8_f32'),
         ('f64', 'NA', 'auto', 'f64'), ('two_grids', 'NA', 'f64', 'f64_split')]
CASE_IDS = ['%s-%s-%s' % (c[0], c[1], c[3]) for c in CASES]


def lookup_points(L, seed, n_random=2000):
    """Part A's points for the lookups L: the per-axis classes of rhs_f32_numpy.axis_points on the static grid (n_random random
    points) and on the wind, thermo and bathymetry grids (a tenth of that each), plus the interiors of up to 150 all-land and 150
    all-sea cells of the static grid.  Returns lon, lat (float64 holding float32 values) and the all-land mask."""
    R = np.float32
    lon, lat = rn.paired_points(L.hx.x, L.hy.x, R, seed, n_random)
    lons, lats = [lon], [lat]
    for k, g in enumerate('wtb'):
        a, b = rn.paired_points(L.axes[g][0].x, L.axes[g][1].x, R, seed + 1 + k, n_random // 10)
        lons.append(a); lats.append(b)
    n0 = sum(len(x) for x in lons)
    P = L.land
    rng = np.random.default_rng(seed + 9)
    n_land = 0
    for val in (1, 0):
        full = (P[:-1, :-1] == val) & (P[1:, :-1] == val) & (P[:-1, 1:] == val) & (P[1:, 1:] == val)
        iy, ix = np.nonzero(full)
        pick = rng.choice(iy.size, size=min(150, iy.size), replace=False)
        for rep in range(4):
            fx, fy = rng.uniform(0.02, 0.98, pick.size), rng.uniform(0.02, 0.98, pick.size)
            x0, x1 = L.hx.x[ix[pick]].astype(np.float64), L.hx.x[ix[pick] + 1].astype(np.float64)
            y0, y1 = L.hy.x[iy[pick]].astype(np.float64), L.hy.x[iy[pick] + 1].astype(np.float64)
            lons.append(rn.f32(x0 + fx * (x1 - x0))); lats.append(rn.f32(y0 + fy * (y1 - y0)))
            if val == 1:
                n_land += pick.size
    lon, lat = np.concatenate(lons), np.concatenate(lats)
    all_land = np.zeros(lon.size, bool)
    all_land[n0:n0 + n_land] = True
    return lon, lat, all_land


def _oracle_lookups(cme, lon, lat):
    from oracle import c_oracle
    lib = c_oracle.lib()

    def bl(g, plane):
        return np.array([lib.orc_bilinear(C.byref(g), plane, float(a), float(b)) for a, b in zip(lon, lat)])
    c = cme.c
    return np.stack([bl(c.wg, c.mean[k]) for k in range(4)] + [bl(c.wg, c.cov[k]) for k in range(10)] +
                    [bl(c.tg, getattr(c, n)) for n in ('vpot', 'chi', 'mld', 'strat')] + [bl(c.hg, c.land), bl(c.bg, c.bathy)], axis=1)


# ------------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize('case', [CASES[0], CASES[1], CASES[2], CASES[3], CASES[6]], ids=[CASE_IDS[i] for i in (0, 1, 2, 3, 6)])
def test_restatement_fp64_equals_c_oracle_bilinear(envs, case):
    """The float64 mode of the restatement — the same code the float32 comparison runs — equals c_oracle.bilinear (FITPACK's
    arithmetic, pinned to the reference by tests/test_oracle_golden.py) bit for bit on part A's point classes: affine axes
    (golden), two grids (gfdl), the general knot walk (gaussian), land and bathymetry on different grids (two_grids)."""
    from oracle import c_oracle
    name, basin = case[0], case[1]
    env = envs(name)
    L = rn.Lookups(env, basin, SLOT, np.float64)
    lon, lat, _ = lookup_points(L, seed=3, n_random=150)
    assert L.affine == (name != 'gaussian')
    got = L(lon, lat)
    ref = _oracle_lookups(c_oracle.CMonthEnv(env, basin, SLOT), lon, lat)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (got != ref).sum(axis=0)
    # the float32 mode is the same code on float32 arrays: it stays float32 throughout and stays within float32 round-off of it
    L32 = rn.Lookups(env, basin, SLOT, np.float32)
    g32 = L32(lon, lat)
    assert g32.dtype == np.float32
    scale = np.abs(ref).max(axis=0) + 1e-30
    assert (np.abs(g32 - ref) / scale).max() < 2e-5


def _draw(basin, n, seed):
    from oracle.scipy_port import BASIN_BOUNDS
    x0, y0, x1, y1 = BASIN_BOUNDS[basin]
    rng = np.random.default_rng(seed)
    lon, lat = rng.uniform(x0, x1, n), rng.uniform(max(y0, -77.0), min(y1, 77.0), n)
    v, m, t = rng.uniform(1, 80, n), rng.uniform(0.02, 1, n), rng.uniform(0, 15 * 86400.0, n)
    return t, rn.f32(lon), rn.f32(lat), rn.f32(v), rn.f32(m)


_C_CACHE = {}


def continuous_reference(env, basin, Fs):
    """Part C's reference for one basin, computed once per (basin, table) and left unchanged: the 20 000 draws, the selection,
    the oracle's outputs on the float-rounded data, the twin response and the magnitudes."""
    from oracle import c_oracle
    from oracle.scipy_port import Params
    key = (basin, Fs.tobytes())
    if key not in _C_CACHE:
        env32, prm32, Fs32 = rn.env_f32(env), rn.params_f32(Params()), rn.f32(Fs)
        L64 = rn.Lookups(env32, basin, SLOT, np.float64)
        cme = c_oracle.CMonthEnv(env32, basin, SLOT)
        t, lon, lat, v, m = _draw(basin, 20000, seed=300 + len(basin) + ord(basin[0]))
        keep, parts = rn.select_continuous(L64, lon, lat)
        t, lon, lat, v, m = (x[keep] for x in (t, lon, lat, v, m))
        ref = rn.oracle_outputs(cme, prm32, Fs32, H_BL, t, lon, lat, v, m)
        twin = rn.twin_response(cme, prm32, Fs32, H_BL, t, lon, lat, v, m, ref)
        mag = rn.magnitudes(L64, prm32, Fs32, H_BL, t, lon, lat, v, m, ref)
        _C_CACHE[key] = dict(env32=env32, prm32=prm32, Fs32=Fs32, cme=cme, L64=L64, pts=(t, lon, lat, v, m), ref=ref, twin=twin, mag=mag,
                             kept=float(keep.mean()), parts={k: float(x.mean()) for k, x in parts.items()})
    return _C_CACHE[key]


def check_continuous(got, c):
    """max over the points of the normalised error per output, and the fraction of points over C_BOUNDS per output"""
    e = rn.normalised_error(got, c['ref'], c['twin'], c['mag'])
    bound = np.array([C_BOUNDS[k] for k in rn.OUTPUTS])
    return e.max(axis=0), (e > bound).mean(axis=0), (e > bound).any(axis=1).mean()


def test_continuous_checker_is_not_vacuous(golden_env):
    """Part C's checker on its own, without a GPU: the undisturbed oracle passes (error 0), and the oracle's output with ONE
    relative defect of 2^-14 planted — in Ck (drives dv, dm), u_beta (dlon), the chi plane (dm), the forcing table (envw, dlon,
    dlat) — fails the final bounds on at least 1 % of the points.  Also: the yardstick is of the order of float32 round-off."""
    from oracle import c_oracle
    Fs = c_oracle.fourier_table(_phases())
    c = continuous_reference(golden_env, 'NA', Fs)
    t, lon, lat, v, m = c['pts']
    assert len(t) >= 10000, c['parts']
    mx, frac, any_frac = check_continuous(c['ref'].copy(), c)
    assert mx.max() == 0.0 and any_frac == 0.0
    rel = (c['twin'] + rn.EPS32 * c['mag']) / np.maximum(np.abs(c['ref']), 1e-300)
    print('kept %.1f %% of the draws %s; yardstick / |value|: median %s' % (100 * c['kept'], c['parts'], ' '.join('%.1e' % x for x in np.median(rel, axis=0))))
    assert (np.median(rel, axis=0) < 1e-5).all()
    planted = {
        'Ck': (dataclasses.replace(c['prm32'], Ck=c['prm32'].Ck * (1 + PLANT)), c['cme'], c['Fs32'], ('dv', 'dm')),
        'u_beta': (dataclasses.replace(c['prm32'], u_beta=c['prm32'].u_beta * (1 + PLANT)), c['cme'], c['Fs32'], ('dlon',)),
        'chi': (c['prm32'], c_oracle.CMonthEnv(dataclasses.replace(c['env32'], chi=c['env32'].chi * (1 + PLANT)), 'NA', SLOT), c['Fs32'], ('dm',)),
        'Fs': (c['prm32'], c['cme'], c['Fs32'] * (1 + PLANT), ('envw0', 'envw1', 'envw2', 'envw3', 'dlon', 'dlat')),
    }
    for name, (prm, cme, Fs_p, drives) in planted.items():
        bad = rn.oracle_outputs(cme, prm, Fs_p, H_BL, t, lon, lat, v, m)
        mx, frac, any_frac = check_continuous(bad, c)
        print('planted %-6s: fraction of points over the bound per output %s, any %.3f' % (name, np.array2string(frac, precision=3), any_frac))
        assert any_frac >= 0.01, (name, any_frac)
        assert max(frac[rn.OUTPUTS.index(k)] for k in drives) >= 0.01, (name, frac)


# ------------------------------------------------------------------------------------------------------------------ GPU tests
def _engine(basin, env, store='auto'):
    import types
    from tropical_cyclone_risk_amd import namelist
    from tropical_cyclone_risk_amd.engine import TCEngine
    nl = types.SimpleNamespace(**{k: getattr(namelist, k) for k in dir(namelist) if not k.startswith('__')})
    nl.gpu_static_store = store
    return TCEngine(basin, device=0, nl=nl).stage_env(env)


@pytest.fixture(scope='module')
def golden_engines(golden_env, built_lib):
    cache = {}

    def get(basin):
        if basin not in cache:
            cache[basin] = _engine(basin, golden_env)
        return cache[basin]
    yield get
    for e in cache.values():
        e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_lookups_bit_for_bit(envs, built_lib, case):
    """A.  aux[:, :20] of the float probe equals the float32 restatement on the bit patterns, and the decision bits follow the
    restated values: bit 0 = restated land == 1, bit 1 = restated vpot != 0.  One context per static storage mode (pack16,
    pack64, u8 + f32, f64, f64 split — the last forced with gpu_static_store = 'f64'), per axis kind (affine; 'gaussian': the
    general knot walk on every axis) and for the two wind / thermo grid arrangements (one grid; 'gfdl': two).  Prints how many of
    the points inside all-land cells give land != 1 in float32; what is asserted is equality with the restatement, not a rate."""
    name, basin, store, mode = case
    env = envs(name)
    L = rn.Lookups(env, basin, SLOT, np.float32)
    lon, lat, all_land = lookup_points(L, seed=11)
    assert lon.size <= 20000 and all_land.sum() >= 100
    want = L(lon, lat)
    rng = np.random.default_rng(5)
    n = lon.size
    v, m, t = rng.uniform(1, 80, n), rng.uniform(0.02, 1, n), rng.uniform(0, 15 * 86400.0, n)
    eng = _engine(basin, env, store)
    Fs = eng.fourier_table(_phases()[None])[0]
    _, _, _, aux = eng.probe_rhs(SLOT, H_BL, Fs, t, lon, lat, v, m, dtype='f32', aux=True)
    got_mode = eng.static_info()[0]
    eng.close()
    assert got_mode == mode and L.affine == (name != 'gaussian')
    assert np.array_equal(aux[:, :20], aux[:, :20].astype(np.float32).astype(np.float64))       # float values, widened
    diff = _bits(aux[:, :20]) != _bits(want)
    assert not diff.any(), ('lookups differ from the float32 restatement', diff.sum(axis=0), np.flatnonzero(diff.any(axis=1))[:8])
    dec = aux[:, 22].astype(np.int64)
    assert np.array_equal(dec & 1, (want[:, 18] == np.float32(1)).astype(np.int64))
    assert np.array_equal((dec >> 1) & 1, (want[:, 14] != np.float32(0)).astype(np.int64))
    miss = int((want[all_land, 18] != np.float32(1)).sum())
    print('%s: %d points, %d in all-land cells of which %d give land != 1 in float32 (restatement and kernel alike)'
          % ('-'.join(case[:2] + (mode,)), n, int(all_land.sum()), miss))


@pytest.mark.gpu
def test_branches_take_the_oracles_side(golden_env, golden_engines):
    """B.  Points built to sit clearly on one side of each discrete branch (chosen with the fp64 oracle on the float-rounded
    data): the fp32 evaluation takes the oracle's branch and gives the exact constants.
      * |lat| >= 80: dlon = dlat = 0 and zero winds in the RHS — so dm = ck_h ((1 - m) v - 0 m), restated in float32;
      * NaN lon: zero env winds;
      * inside golden_env's zero-covariance patch: the Cholesky factorisation fails, envw == 0 exactly;
      * all-land cells where the restated land == 1: PI = 0, so dv = ck_h (0 - (1 - gamma m^3) v^2) and alpha restated;
      * bathymetry >= 0, -h_m <= bathymetry, stratification == 0: alpha == 1.0 exactly;
      * v = 0: alpha's `/ v` is inf where PI uT > 0 (alpha = 1 - 0.87 exp(-100), dv = ck_h alpha beta PI^2 m^3 > 0) and NaN
        where it is 0 / 0 (dv = NaN -> 0, coupled_fast.py:150): dv == 0 exactly where the oracle's is, finite and equal to
        float32 round-off elsewhere."""
    from oracle import c_oracle
    from oracle.scipy_port import Params
    R = np.float32
    prm32 = rn.params_f32(Params())
    rng = np.random.default_rng(23)
    ph = _phases()

    def run(basin, t, lon, lat, v, m, eng=None, env=golden_env):
        eng = eng or golden_engines(basin)
        Fs = eng.fourier_table(ph[None])[0]
        d, w, a, aux = eng.probe_rhs(SLOT, H_BL, Fs, t, lon, lat, v, m, dtype='f32', aux=True)
        cme = c_oracle.CMonthEnv(rn.env_f32(env), basin, SLOT)
        with np.errstate(all='ignore'):
            ref = rn.oracle_outputs(cme, prm32, rn.f32(Fs), H_BL, t, lon, lat, v, m)
        return d, w, a, aux, ref

    ck_h = R(0.5) * R(prm32.Ck) / R(H_BL)
    eps, kap = R(prm32.epsilon), R(prm32.kappa)

    # ---- polar
    lat = rn.f32(np.concatenate([[80.0, -80.0, 85.0, -83.5, 89.0], rng.uniform(80, 90, 60) * rng.choice([-1, 1], 60)]))
    n = lat.size
    lon, v, m, t = rn.f32(rng.uniform(5, 355, n)), rn.f32(rng.uniform(1, 80, n)), rn.f32(rng.uniform(0.02, 1, n)), rng.uniform(0, 15 * 86400.0, n)
    d, w, a, aux, ref = run('GL', t, lon, lat, v, m)
    assert (d[:, 0] == 0).all() and (d[:, 1] == 0).all() and (ref[:, 0] == 0).all() and (ref[:, 1] == 0).all()
    v32, m32 = v.astype(R), m.astype(R)
    dm = ck_h * ((R(1) - m32) * v32 - (R(0.0) * aux[:, 21].astype(R)) * m32)
    assert np.array_equal(_bits(d[:, 3]), _bits(dm))
    # one float32 below 80 degrees the storm still moves
    lat2 = np.nextafter(R(80), R(0)).astype(np.float64) * np.array([1.0, -1.0])
    d2 = run('GL', t[:2], lon[:2], lat2, v[:2], m[:2])[0]
    assert (d2[:, 1] != 0).all()

    # ---- NaN lon
    lon_nan = np.full(8, np.nan)
    d, w, a, aux, ref = run('NA', t[:8], lon_nan, rn.f32(rng.uniform(5, 55, 8)), v[:8], m[:8])
    assert (w == 0).all() and (ref[:, 4:8] == 0).all()

    # ---- zero-covariance patch (300..312 E, 22..30 N of month 9): strictly inside, on its knots too
    n = 300
    lon = rn.f32(np.concatenate([rng.uniform(300.0, 312.0, n - 4), [300.0, 312.0, 305.0, 306.5]]))
    lat = rn.f32(np.concatenate([rng.uniform(22.0, 30.0, n - 4), [22.0, 30.0, 25.0, 29.5]]))
    v, m, t = rn.f32(rng.uniform(1, 80, n)), rn.f32(rng.uniform(0.02, 1, n)), rng.uniform(0, 15 * 86400.0, n)
    d, w, a, aux, ref = run('NA', t, lon, lat, v, m)
    assert (ref[:, 4:8] == 0).all() and (aux[:, 4] == 0).all()          # the oracle's factorisation fails on every one of them
    assert (w == 0).all()
    # ... and the RHS went on with zero winds: dm = ck_h ((1 - m) v - 0 chi m)
    v32, m32 = v.astype(R), m.astype(R)
    dm = ck_h * ((R(1) - m32) * v32 - (R(0.0) * aux[:, 21].astype(R)) * m32)
    assert np.array_equal(_bits(d[:, 3]), _bits(dm))

    # ---- land, shelf, stratification, v = 0: classes picked from random NA points with the oracle's lookups on the float-rounded data
    L64 = rn.Lookups(rn.env_f32(golden_env), 'NA', SLOT, np.float64)
    L32 = rn.Lookups(golden_env, 'NA', SLOT, np.float32)
    t, lon, lat, v, m = _draw('NA', 100000, seed=77)
    q = L64(lon, lat)
    q32 = L32(lon, lat)
    (ix, _, _), (iy, _, _) = L64.cells('h', lon, lat)
    P = L64.land
    all_land = (P[iy, ix] == 1) & (P[iy + 1, ix] == 1) & (P[iy, ix + 1] == 1) & (P[iy + 1, ix + 1] == 1)
    all_sea = (P[iy, ix] == 0) & (P[iy + 1, ix] == 0) & (P[iy, ix + 1] == 0) & (P[iy + 1, ix + 1] == 0)
    bathy, h_m, gam = q[:, 19], q[:, 16], q[:, 17]
    cls = dict(land=all_land & (q32[:, 18] == R(1)) & ((bathy >= 1.0) | (gam > 0.01) | (gam == 0)),
               bathy_pos=bathy >= 1.0,
               shelf=all_sea & (bathy < -0.5) & (-h_m <= bathy - 0.5))
    pick = np.concatenate([np.flatnonzero(c)[:400] for c in cls.values()])
    assert all(c.sum() >= 20 for c in cls.values()), {k: int(c.sum()) for k, c in cls.items()}
    t, lon, lat, v, m = (x[pick] for x in (t, lon, lat, v, m))
    cls = {k: c[pick] for k, c in cls.items()}
    d, w, a, aux, ref = run('NA', t, lon, lat, v, m)
    for k in ('bathy_pos', 'shelf'):
        assert (a[cls[k]] == 1.0).all() and (ref[cls[k], 8] == 1.0).all(), k
    ld = cls['land']
    assert (aux[ld, 20] == 0).all() and ((aux[ld, 22].astype(int) & 1) == 1).all()          # PI in use is 0: `land == 1`
    no_mix = (aux[ld, 19] >= 0) | (-aux[ld, 16] <= aux[ld, 19]) | (aux[ld, 17] == 0)
    al = np.where(no_mix, R(1.0), R(1) - R(0.87) * R(1.0)).astype(R)                      # z = 0: exp(-0) = 1
    assert np.array_equal(_bits(a[ld]), _bits(al))
    v32, m32 = v[ld].astype(R), m[ld].astype(R)
    m3 = m32 * m32 * m32
    gamma = eps + al * kap
    dv = ck_h * (R(0.0) - (R(1) - gamma * m3) * (v32 * v32))
    assert np.array_equal(_bits(d[ld, 2]), _bits(dv))
    # ---- stratification == 0 over deep open water (golden_env's coasts leave no such point: a copy with a zeroed patch, 320..330 E, 10..20 N)
    strat = golden_env.strat.copy()
    strat[SLOT][np.ix_((golden_env.lat >= 10) & (golden_env.lat <= 20), (golden_env.lon >= 320) & (golden_env.lon <= 330))] = 0.0
    env_ns = dataclasses.replace(golden_env, strat=strat)
    eng_ns = _engine('NA', env_ns)
    k = 200
    lo_ns, la_ns = rn.f32(np.concatenate([rng.uniform(320, 330, k - 2), [320.0, 330.0]])), rn.f32(np.concatenate([rng.uniform(10, 20, k - 2), [10.0, 20.0]]))
    d_ns, _, a_ns, aux_ns, ref_ns = run('NA', t[:k], lo_ns, la_ns, v[:k], m[:k], eng=eng_ns, env=env_ns)
    eng_ns.close()
    assert (aux_ns[:, 17] == 0).all() and (aux_ns[:, 19] < -1000).all() and (-aux_ns[:, 16] > aux_ns[:, 19]).all()      # gam == 0 alone decides
    assert (a_ns == 1.0).all() and (ref_ns[:, 8] == 1.0).all()
    # ---- v = 0 at the same points
    v0 = np.zeros_like(v)
    d, w, a, aux, ref = run('NA', t, lon, lat, v0, m)
    assert np.isfinite(d).all() and np.array_equal(d[:, 2] == 0, ref[:, 2] == 0)
    nz = ref[:, 2] != 0
    assert nz.sum() >= 20 and (np.abs(d[nz, 2] - ref[nz, 2]) <= 1e-5 * np.abs(ref[nz, 2])).all()
    assert np.array_equal(a == 1.0, ref[:, 8] == 1.0)


@pytest.mark.gpu
def test_continuous_rhs_against_oracle(golden_env, golden_engines):
    """C.  20 000 random points per basin (NA, GL; month 9), reduced by the oracle to those at which no decision can differ
    (rhs_f32_numpy.select_continuous): at least 10 000 remain, no decision differs on them, and every output stays within
    C_BOUNDS of the oracle in units of twin + 2^-24 mag (rhs_f32_numpy.twin_response / magnitudes).
    Measured on the MI355X, maximum over both basins (14 995 NA + 14 622 GL points) of the normalised error — C_MEASURED:
        dlon 5.30  dlat 1.95  dv 1.65  dm 1.76  envw 1.96 / 2.15 / 2.73 / 2.22  alpha 1.16
    C_BOUNDS = 4 x that, rounded up to one digit:
        dlon 30    dlat 8     dv 7     dm 8     envw 8 / 9 / 20 / 9              alpha 5"""
    worst = np.zeros(9)
    for basin in ('NA', 'GL'):
        eng = golden_engines(basin)
        Fs = eng.fourier_table(_phases()[None])[0]
        c = continuous_reference(golden_env, basin, Fs)
        t, lon, lat, v, m = c['pts']
        assert len(t) >= 10000, (basin, c['kept'], c['parts'])
        d, w, a, aux = eng.probe_rhs(SLOT, H_BL, Fs, t, lon, lat, v, m, dtype='f32', aux=True)
        got = np.concatenate([d, w, a[:, None]], axis=1)
        ref = c['ref']
        dec = aux[:, 22].astype(np.int64)
        assert ((dec & 1) == 0).all() and (((dec >> 1) & 1) == 1).all()
        # (alpha = 1 - 0.87 exp(-z) rounds to 1 in float32 for z > 17.3 and in float64 for z > 37: `alpha < 1` is a matter of
        # precision on the mixing branch, not a decision — the normalised error of alpha below holds it; no value exceeds 1)
        assert (a <= 1).all() and (ref[:, 8] <= 1).all() and np.array_equal(a[ref[:, 8] < 0.99] < 1, np.ones((ref[:, 8] < 0.99).sum(), bool))
        assert np.array_equal((w != 0).any(axis=1), (ref[:, 4:8] != 0).any(axis=1)) and (w != 0).any(axis=1).all()
        mx, frac, any_frac = check_continuous(got, c)
        print('%s: %d points (%.1f %% of the draws); max normalised error %s' % (basin, len(t), 100 * c['kept'], dict(zip(rn.OUTPUTS, np.round(mx, 2)))))
        worst = np.maximum(worst, mx)
    print('both basins: max normalised error %s' % dict(zip(rn.OUTPUTS, np.round(worst, 2))))
    for k, x in zip(rn.OUTPUTS, worst):
        assert x <= C_BOUNDS[k], (k, x, C_BOUNDS[k])


@pytest.mark.gpu
def test_float_helpers_against_numpy(built_lib):
    """D.  The float instantiations of the arithmetic helpers (tcr_probe_math_host fn 6-12), 400 000 operands each over the ranges
    of the fp64 test (tests/test_gpu_parity.py::test_integrator_arithmetic_helpers_against_numpy):
      * qdiv_nz / qsqrt / qsqrt_pos<float>: NumPy float32 division and sqrt bit for bit;
      * pow(a, -0.2f), pow(g, -0.4f), cos on [-pi / 2, pi / 2], exp(-x) on [0, 100]: against the 80-bit NumPy value of the same float
        arguments and float exponents; the assertion is the next integer above the measured maximum, at least 2 float ulp (the
        project's libm-class limit, tcr_device.h "Arithmetic policy").
    Measured on the MI355X, maximum in float ulp: pow(a, -0.2f) 1.259, pow(g, -0.4f) 1.231, cos 1.530, exp(-x) 0.816 — so the
    limit is 2 for each (D_LIMIT)."""
    from tropical_cyclone_risk_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.tcr_ctx_create(0, C.byref(h)) == 0
    R, LD = np.float32, np.longdouble

    def run(fn, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        out = np.empty_like(a)
        bb = np.ascontiguousarray(b, dtype=np.float64) if b is not None else None
        rc = lib.tcr_probe_math_host(h, fn, a.size, a.ctypes.data_as(_lib.DP), bb.ctypes.data_as(_lib.DP) if bb is not None else None,
                                     out.ctypes.data_as(_lib.DP))
        assert rc == 0, lib.tcr_last_error(h).decode()
        assert np.array_equal(out, out.astype(R).astype(np.float64), equal_nan=True)      # float results, widened
        return out.astype(R)

    def ulps(got, want_ld):
        want = want_ld.astype(R)
        return np.abs((got.astype(LD) - want_ld) / np.spacing(np.abs(want)).astype(LD)).astype(np.float64)
    rng = np.random.default_rng(6)
    n = 400_000
    # ---- division: dividends of either sign over the float range the path has, the divisors of the fp64 test
    a = (rng.normal(size=n) * 10.0 ** rng.uniform(-20, 20, n)).astype(R)
    b = np.concatenate([rng.uniform(0.17, 1.0, n // 4), rng.uniform(500, 3000, n // 4), 10.0 ** rng.uniform(-6, 2, n // 4),
                        rng.uniform(0.5, 30, n - 3 * (n // 4))]).astype(R)
    with np.errstate(over='ignore', under='ignore'):
        want = a / b
    q = run(6, a, b)
    assert np.array_equal(_bits(q), _bits(want)), 'qdiv_nz<float> differs from IEEE division on %d of %d operands' % ((_bits(q) != _bits(want)).sum(), n)
    assert np.isnan(run(6, [np.nan, 1.0], [2.0, np.nan])).all()
    # ---- square roots
    x = (10.0 ** rng.uniform(-12, 8, n)).astype(R)
    for fn in (7, 8):
        assert np.array_equal(_bits(run(fn, x)), _bits(np.sqrt(x))), fn
    s = run(7, [0.0, np.inf, -1.0, np.nan, 4.0])
    assert s[0] == 0.0 and s[1] == np.inf and np.isnan(s[2]) and np.isnan(s[3]) and s[4] == 2.0
    # ---- powers with the float exponents the float instantiation raises to
    e = (10.0 ** rng.uniform(-14, 6, n)).astype(R)
    u3 = ulps(run(9, e), np.power(e.astype(LD), LD(R(-0.2)))).max()
    g = (10.0 ** rng.uniform(-4, 3, n)).astype(R)
    u4 = ulps(run(10, g), np.power(g.astype(LD), LD(R(-0.4)))).max()
    sp = run(10, [-1.0, np.nan, 1.0, 32.0])
    assert np.isnan(sp[0]) and np.isnan(sp[1]) and sp[2] == 1.0 and abs(sp[3] - R(0.25)) <= 2 * np.spacing(R(0.25))
    pw = R(0.9) * run(9, [1e-300, 0.0, 1e300, np.nan])          # (1e-300 and 1e300 round to 0 and inf in float)
    assert np.fmin(R(10.0), pw[0]) == 10.0 and np.fmin(R(10.0), pw[1]) == 10.0 and np.fmax(R(0.2), pw[2]) == R(0.2) and np.fmax(R(0.2), pw[3]) == R(0.2)
    # ---- cos on [-pi / 2, pi / 2], exp(-x) on [0, 100]
    xr = (rng.uniform(-90, 90, n) * (np.pi / 180.0)).astype(R)
    xr = xr[np.abs(xr.astype(np.float64)) <= np.pi / 2]
    u5 = ulps(run(11, xr), np.cos(xr.astype(LD))).max()
    c = run(11, [0.0, np.nan])
    assert c[0] == 1.0 and np.isnan(c[1])
    z = rng.uniform(0, 100, n).astype(R)
    u6 = ulps(run(12, z), np.exp(-z.astype(LD))).max()
    ez = run(12, [0.0, 100.0, np.nan])
    assert ez[0] == 1.0 and 0 < ez[1] < 1e-43 and np.isnan(ez[2])
    lib.tcr_ctx_destroy(h)
    print('float helpers: division / sqrt bit-identical on %d operands each; pow(a, -0.2f) %.3f ulp, pow(g, -0.4f) %.3f ulp, '
          'cos %.3f ulp, exp(-x) %.3f ulp' % (n, u3, u4, u5, u6))
    for name, u in (('pow(a, -0.2f)', u3), ('pow(g, -0.4f)', u4), ('cos', u5), ('exp(-x)', u6)):
        assert u <= D_LIMIT[name], (name, u)


# the next integer above the measured maximum, at least 2
D_LIMIT = {'pow(a, -0.2f)': 2.0, 'pow(g, -0.4f)': 2.0, 'cos': 2.0, 'exp(-x)': 2.0}

E_YEAR = 2001         # its first 64 GL candidates: 25 gated, 39 not, none within 1e-3 of the gate (counted with the CPU oracles)


@pytest.mark.gpu
def test_probe_ties_to_the_shipped_kernels(golden_env, golden_engines):
    """E.  64 GL candidates of E_YEAR integrated in fp32 with all rows; per storm the float probe, with that storm's slot, h_bl and
    forcing table, at its emitted (t_j, lon_j, lat_j), j < n_valid: the probe's env winds equal the row's bit for bit (k_emit<float>
    and the probe call the same env_winds<float>), and status == GATED agrees with S chi / PI >= 1 restated in float32 from the
    probe's values at t = 0 (k_integrate<float> may fuse S^2's sum — TCR_FUSE_RK — so storms whose fp64 ratio is within 1e-3 of 1
    are left out: at most 0.5 %, and at least 20 storms fall on each side)."""
    from oracle import c_oracle
    from tropical_cyclone_risk_amd import _lib
    R = np.float32
    eng = golden_engines('GL')
    n = 64
    s = eng.seed(E_YEAR, 0, n)
    storms = {k: s[k] for k in ('lon', 'lat', 'v0', 'm0', 'h_bl', 'month', 'phases')}
    # the gate in fp64 with the CPU oracle
    ratio64 = np.empty(n)
    for i in range(n):
        cme = c_oracle.CMonthEnv(golden_env, 'GL', int(s['month'][i]) - 1)
        one = lambda x: [float(x[i])]
        _, w, _ = c_oracle.rhs_points(cme, c_oracle.fourier_table(s['phases'][i]), float(s['h_bl'][i]), [0.0], one(s['lon']), one(s['lat']), one(s['v0']), one(s['m0']))
        land = c_oracle.bilinear(cme, 'h', 'land', one(s['lon']), one(s['lat']))[0]
        vp = 0.0 if land == 1 else c_oracle.bilinear(cme, 't', 'vpot', one(s['lon']), one(s['lat']))[0]
        chi = c_oracle.bilinear(cme, 't', 'chi', one(s['lon']), one(s['lat']))[0]
        ratio64[i] = np.hypot(w[0, 0] - w[0, 2], w[0, 1] - w[0, 3]) * chi / vp if vp > 0 else 0.0
    clear = np.abs(ratio64 - 1) >= 1e-3
    assert (~clear).sum() <= 0.005 * n and (ratio64[clear] >= 1).sum() >= 20 and (ratio64[clear] < 1).sum() >= 20
    out = eng.integrate(storms, dtype='f32')
    assert out['envw'].dtype == R
    Fs = eng.fourier_table(s['phases'])
    gated = np.zeros(n, bool)
    rows = 0
    for i in range(n):
        nv = int(out['n_valid'][i])
        t = np.concatenate([[0.0], eng.t_s[:nv]])
        lon = np.concatenate([[float(R(s['lon'][i]))], out['lon'][i, :nv].astype(np.float64)])
        lat = np.concatenate([[float(R(s['lat'][i]))], out['lat'][i, :nv].astype(np.float64)])
        v = np.concatenate([[s['v0'][i]], out['v'][i, :nv].astype(np.float64)])
        m = np.concatenate([[s['m0'][i]], out['m'][i, :nv].astype(np.float64)])
        _, w, _, aux = eng.probe_rhs(int(s['month'][i]) - 1, float(s['h_bl'][i]), Fs[i], t, lon, lat, v, m, dtype='f32', aux=True)
        assert np.array_equal(_bits(w[1:]), _bits(out['envw'][i, :nv])), (i, nv)
        rows += nv
        w0 = w[0].astype(R)
        du, dw = w0[0] - w0[2], w0[1] - w0[3]
        shear = np.sqrt(du * du + dw * dw)
        vp, chi = R(aux[0, 20]), R(aux[0, 21])
        with np.errstate(divide='ignore', invalid='ignore'):
            gated[i] = bool(vp > 0 and shear * chi / vp >= R(1))
    assert rows > 1000
    assert np.array_equal((out['status'] == _lib.STATUS_GATED)[clear], gated[clear])
    assert np.array_equal(gated[clear], ratio64[clear] >= 1)
    print('E: %d rows bit-identical; %d gated, %d not, %d left out' % (rows, gated[clear].sum(), (~gated[clear]).sum(), (~clear).sum()))
