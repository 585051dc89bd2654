"""Soundings that reach the branches of the potential-intensity fold (csrc/tcr_thermo.hip, oracle/thermo_oracle.py).

`family` starts from the soundings of tests/golden/make_golden_thermo.py (latitude-dependent SST, power-law troposphere,
isothermal stratosphere, noise) and gives random shares of the columns the features that decide which level the fold
picks: a parcel saturated at the lowest level, no condensation at all, hits in several separate runs, a last hit at the
top level, levels above the entropy table's pressure axis, entropies off its entropy axis, NaNs, zeros.
tests/test_thermo.py's census asserts that the shares below do reach them.
"""
import numpy as np

# ERA5's 37 pressure levels, lowest (highest pressure) first
ERA5_LEVELS_PA = 100.0 * np.array([1000, 975, 950, 925, 900, 875, 850, 825, 800, 775, 750, 700, 650, 600, 550, 500, 450, 400, 350,
                                   300, 250, 225, 200, 175, 150, 125, 100, 70, 50, 30, 20, 10, 7, 5, 3, 2, 1], dtype=np.float64)

# the axes of a handful of levels: two is the fewest the ABI takes; the last has half its levels above the table
FEW_LEVELS_PA = {'l2': 100.0 * np.array([1000.0, 500.0]), 'l3': 100.0 * np.array([950.0, 600.0, 200.0]),
                 'l4': 100.0 * np.array([1010.0, 850.0, 10.0, 1.0])}


def rs_like(T, p):
    tc = T - 273.0
    es = 610.94 * np.exp(np.minimum(17.625 * tc / (tc + 243.04), 10))
    return 0.622 * es / (p - es)


def dry_to_the_top(rng, p, T, r, cols):
    """Columns whose unsaturated parcel shows the reference's top-level rule (the top level is on the moist adiabat whatever
    the LCL): moisture so small that the LCL lies above every level, an environment that is a dry adiabat 1-4 K colder
    than the parcel's up to the level below the top, so the parcel's last hit is that level with a buoyancy that is not
    zero, and a top too warm for either parcel.  The parcel's temperature at the top then enters x through the outflow
    interpolation alone.  Nothing to do on two levels: the level below the top is level 0, where the buoyancy is 0."""
    L = len(p)
    if L < 3:
        return
    r[:, cols] = 1e-80
    T[1:L - 1, cols] = T[0, cols][None] * (p[1:L - 1, None] / p[0]) ** (287.04 / 1005.04) - rng.uniform(1, 4, size=int(cols.sum()))[None]
    T[L - 1, cols] = 0.85 * T[0, cols]


def family(rng, n, p):
    """sst [n], psl [n], T [L, n], r [L, n] on the levels p (Pa, lowest first)."""
    p = np.asarray(p, dtype=np.float64)
    L = len(p)
    pc = p[:, None]
    pick = lambda share: rng.random(n) < share
    # nine columns in ten lie within 35 degrees of the equator, where the product works; the rest reach to 75
    lat = rng.uniform(-1, 1, size=n) * np.where(pick(0.9), 35.0, 75.0)
    sst = 302.0 - 28.0 * (np.abs(lat) / 75.0) ** 1.6 + rng.normal(0, 0.8, size=n)
    t_ns = sst - rng.uniform(0.3, 2.5, size=n)
    gamma = rng.uniform(0.17, 0.22, size=n)
    T = t_ns[None] * (pc / p[0]) ** gamma[None]
    T = np.maximum(T, rng.uniform(195, 215, size=n)[None])                 # isothermal stratosphere
    # stratospheric warming above 100 hPa, per e-fold of pressure
    w = np.where(pick(0.5), rng.uniform(4, 14, size=n), 0.0)
    T = T + w[None] * np.maximum(np.log(10000.0 / pc), 0.0)
    T = T + rng.normal(0, 0.3, size=T.shape)
    # a warm layer 1-3 levels deep: the parcel's hits fall into two or more separate runs
    for c in np.nonzero(pick(0.4))[0]:
        k0 = int(rng.integers(1, max(L - 1, 2)))
        T[k0:k0 + int(rng.integers(1, 4)), c] += rng.uniform(2, 12)
    # the top six levels colder by 20-60 K; in one such column in three at 60-110 K, colder than the 100-160 K that the table
    # gives a parcel at its lowest pressure, which alone makes the parcel's last hit the top level itself
    cold = pick(0.09)
    drop = rng.uniform(20, 60, size=n)
    T[-min(6, L - 1):, cold] -= drop[None, cold]
    deep = cold & pick(0.33)
    T[-min(6, L - 1):, deep] = rng.uniform(60, 110, size=(min(6, L - 1), int(deep.sum())))
    # a warm environment: no buoyancy anywhere
    warm = pick(0.05)
    T[:, warm] += rng.uniform(3, 15, size=int(warm.sum()))[None]
    # a surface inversion of polar-night strength: air at the lowest level so cold that its entropy is off the table's axis
    inv = pick(0.02)
    T[0, inv] = rng.uniform(245, 268, size=int(inv.sum()))
    rh = np.clip(rng.uniform(0.55, 0.9, size=n)[None] * (pc / p[0]) ** rng.uniform(0.5, 2.0, size=n)[None], 0.02, 0.98)
    r = rh * rs_like(T, pc)
    psl = 101000.0 + rng.normal(0, 600, size=n)
    low = pick(0.05)                                                       # surface pressure below the lowest level's
    psl[low] = rng.uniform(60000.0, 90000.0, size=int(low.sum()))
    r[:, pick(0.05)] *= 0.02                                               # very dry: LCL far aloft
    for value, share in ((0.0, 0.01), (273.15, 0.01), (271.3, 0.01), (310.0, 0.015)):
        sst[pick(share)] = value
    # surface mixing ratio at 1.0-1.3 x the saturation value the LCL routine measures it against: saturated at level 0
    sat = pick(0.06)
    r[0, sat] = rs_like(sst[sat], psl[sat]) * rng.uniform(1.0, 1.3, size=int(sat.sum()))
    dry_to_the_top(rng, p, T, r, pick(0.02))
    r[0, pick(0.02)] = 0.0
    for c in np.nonzero(pick(0.02))[0]:
        T[int(rng.integers(0, L)), c] = np.nan
    for c in np.nonzero(pick(0.02))[0]:
        r[int(rng.integers(0, L)), c] = np.nan
    return sst, psl, T, r


def few_levels(rng, n):
    """tag -> (p, sst, psl, T, r): n family columns on each axis of FEW_LEVELS_PA.  On so few levels the saturated parcel is
    nearly always still buoyant at the top level, which leaves PI = 0 whatever the fold does below.  So half of the columns
    are warmed above the lowest level, which puts the last hit below the top, a quarter are dried, and one in seven is
    made `dry_to_the_top` (on three and four levels; on two the level below the top is level 0, where the buoyancy is 0)."""
    out = {}
    for tag, p in FEW_LEVELS_PA.items():
        sst, psl, T, r = family(rng, n, p)
        warm = rng.random(n) < 0.5
        T[1:, warm] += rng.uniform(5, 25, size=int(warm.sum()))[None]
        r[:, rng.random(n) < 0.25] *= 0.02
        dry_to_the_top(rng, p, T, r, rng.random(n) < 0.15)
        out[tag] = (p, sst, psl, T, r)
    return out


def subset_table(p, s, T, rng, n_p=60, n_s=70):
    """The entropy table on a random non-uniform subset of its own knots, first and last kept: a piecewise-bilinear
    table in its own right whose knots no uniform-grid guess finds."""
    def sub(n, m):
        return np.sort(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), size=m - 2, replace=False)]))
    i, j = sub(len(p), n_p), sub(len(s), n_s)
    return np.ascontiguousarray(p[i]), np.ascontiguousarray(s[j]), np.ascontiguousarray(T[np.ix_(i, j)])
