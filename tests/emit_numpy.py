"""The emission stage restated for tests/test_emit.py: what k_emit and k_flags make of one storm's emitted rows (NumPy only).

All inputs are the rows of ONE storm as they were emitted — lon[:n], lat[:n], v[:n], envw[:n, 4] — widened to float64, so nothing is
integrated on the reference side and nothing is amplified:
  vmax_ref      oracle.scipy_port.max_wind on those rows (the port of axi_to_max_wind and calc_translational_speed, pinned to the
                reference's golden tracks); it is called, not restated;
  vmax_bound    a first-order forward error bound of the device's evaluation of the same quantity in type R, term by term;
  vmax_in       the device's formulation (tcr_kernels.hip: vmax_at and the neighbour rules of k_emit) evaluated with NumPy in
                type R: the CPU stand-in for the kernel and the host of the planted defects;
  accept_flags  is_tc and accepted from the rows, exactly.
"""
import numpy as np

from oracle import scipy_port as sp
from tests import rk_steps_numpy as rk

EARTH_R = sp.EARTH_R
WAVE, BLOCK = 64, 128                  # lanes of a wave, threads of a k_emit workgroup (kPostThreads)
GATED = -1

# the planted defects of vmax_in
DEFECTS = ('shuffle_edges',            # (a) lanes 0 / 63 keep what the shuffle gave them: their own sample
           'no_extrapolation',         # (b) one-sided difference, halved, at both ends
           'end_before_fixup',         # (c) the extrapolation at i == n - 1 reads the lower neighbour before lane 0's fix-up
           'G_one',                    # (d) G = 1
           'shear_low_only',           # (e) shear from (w0, w1) alone
           'shear_swapped',            # (f) us and vs swapped
           'neighbour_time',           # (g) lanes 0 / 63 evaluate their outside neighbour at ts(i) instead of ts(i -+ 1)
           'relative')                 # (h) vmax (1 + rel)


def _rows64(lon, lat, v, envw):
    return (np.asarray(lon, np.float64), np.asarray(lat, np.float64), np.asarray(v, np.float64), np.asarray(envw, np.float64).reshape(-1, 4))


def vmax_ref(lon, lat, v, envw, dt_out):
    """scipy_port.max_wind on one storm's rows; NaN for a storm of one sample (no translation speed)"""
    lon, lat, v, envw = _rows64(lon, lat, v, envw)
    with np.errstate(all='ignore'):
        return np.asarray(sp.max_wind(lon, lat, dt_out, v, envw), np.float64).reshape(-1)


def inner_wind(lon, lat, v, envw, dt_out):
    """(Ui, Vi) of tc_wind.py:12-15 in float64 — scipy_port.translation_speed, G and the shear term — and G"""
    lon, lat, v, envw = _rows64(lon, lat, v, envw)
    ut, vt = sp.translation_speed(lon, lat, dt_out)
    G = np.minimum(1., 0.8 + 0.35 * (1. + np.tanh((lat - 35.) / 10.)))
    Ui = G * ut + 0.1 * (envw[:, 0] - envw[:, 2]) * v / 15.
    Vi = G * vt + 0.1 * (envw[:, 1] - envw[:, 3]) * v / 15.
    return Ui, Vi, G


def vmax_identity(lon, lat, v, envw, dt_out):
    """vmax = v + min(|U|, v / 2) with U = (Ui, Vi).  tc_wind.py:16-21 adds to the wind v along U-hat the vector U fac with
    fac = min(1, (v / 2) / |U|): if v / 2 < |U| that is (v / 2) U-hat and the sum is 1.5 v; otherwise fac = 1 and the sum is
    (v + |U|) U-hat.  (|U| = 0: th = -0, the wind is (0, v), the sum v.)  So vmax is 1-Lipschitz in U at fixed v."""
    _, _, v, _ = _rows64(lon, lat, v, envw)
    Ui, Vi, _ = inner_wind(lon, lat, v, envw, dt_out)
    return v + np.minimum(np.hypot(Ui, Vi), 0.5 * v)


def fac_of(lon, lat, v, envw, dt_out):
    """fac = min(1, (v / 2) / |U|) per sample, float64"""
    _, _, v, _ = _rows64(lon, lat, v, envw)
    Ui, Vi, _ = inner_wind(lon, lat, v, envw, dt_out)
    with np.errstate(all='ignore'):
        return np.minimum(1.0, 0.5 * v / np.hypot(Ui, Vi))


def vmax_bound(R, lon, lat, v, envw, dt_out, earth_R=EARTH_R):
    """First-order forward error bound [n] of vmax_at / k_emit evaluated in type R (u = 2^-24 or 2^-53) on exact inputs, from the
    float64 values of the intermediate quantities.  One rounded operation costs u times its result (0.5 ulp), a library call —
    sin, cos, asin, tanh, sqrt, division — 2u times its result (1 ulp), a constant that is not a float (pi / 180, R_earth / 1000,
    0.1, 0.35, 0.8) u times its value.  There is no free constant; what the library calls really cost is absorbed by the test's
    E_BOUND.  With d = pi / 180, K = R_earth / dt_out (the factors R_earth / 1000, 2, 0.5, 1000 / dt_out of a translation speed) and
    lom / lop, lam / lap the lower and upper neighbours in degrees:
      ends      i == 0: lom = 2 lon - lop, i == n - 1: lop = 2 lon - lom (2 x is exact)        e_lom = u |lom|, e_lop = u |lop|
      D    = lop d - lom d           radians first: each product is rounded and d is; the difference cancels
                                                    dD   = u (|lop| + |lom|) d + 2u |D| + (e_lop + e_lom) d
      sb   = sin(D / 2)                             dsb  = |cos(D / 2)| dD / 2 + 2u |sb|
      c    = cos(lat d)                             dc   = |sin(lat d)| 2u |lat d| + 2u |c|
      s    = sqrt(0 + c c (sb sb)) = |c sb|         ds   = |sb| dc + |c| dsb + 3.5u s     (three products halved by the root, the root)
      as   = asin(s)                                das  = ds / sqrt(1 - s^2) + 2u as
      ut   = sgn(lop - lom) K as                    dut  = K das + 5u |ut|                 (R_earth / 1000, its product, x 1000, / dt_out)
      vt:  the same with D' = lap d - lam d, sa = sin(D' / 2), s = sqrt(sa sa) = |sa|: ds = dsa + 2.5u s
      x    = (lat - 35) / 10                        dx   = 3u |x|
      th   = tanh(x)                                dth  = (1 - th^2) dx + 2u |th|
      g    = 0.8 + 0.35 (1 + th)                    dg   = 0.35 (dth + u (1 + th)) + 2u 0.35 (1 + th) + 0.8u + u g
      G    = min(1, g)                              dG   = dg where g < 1 + dg, else 0
      us   = w0 - w2  (vs = w1 - w3)                dus  = u |us|
      t2   = 0.1 us v / 15                          dt2  = (0.1 v / 15) dus + 5u |t2|      (0.1, two products, the division)
      Ui   = G ut + t2                              dUi  = |ut| dG + G dut + u |G ut| + dt2 + u |Ui|
      vmax = v + min(|U|, v / 2), 1-Lipschitz in U (vmax_identity), and constant in U where |U| - |dU| > v / 2
                                                    dvm  = |(dUi, dVi)| (0 where |U| - |dU| > v / 2) + 10u vmax
    The last term counts what vmax_at does with (Ui, Vi, v): |U| = sqrt(Ui Ui + Vi Vi) 3u, fac 5u, Ui / |U| 5u, each of the two
    products of ug 6u and their sum — both have the sign of Ui — 7u, then sqrt(ug ug + vg vg) 7u + 1u + 2u.
    At lon = 300 in float32 the first term of dD is 1e-4 of an hourly displacement of 0.3 degrees and dominates everything else."""
    u = rk.unit_roundoff(R)
    lon, lat, v, envw = _rows64(lon, lat, v, envw)
    n = len(lon)
    if n < 2:
        return np.full(n, np.nan)
    d, K = np.pi / 180.0, earth_R / dt_out

    def speed(x, same_lat):
        xm = np.concatenate([[2 * x[0] - x[1]], x[:-1]])
        xp = np.concatenate([x[1:], [2 * x[-1] - x[-2]]])
        e_m, e_p = np.zeros(n), np.zeros(n)
        e_m[0], e_p[-1] = u * abs(xm[0]), u * abs(xp[-1])
        D = (xp - xm) * d
        dD = u * (np.abs(xp) + np.abs(xm)) * d + 2 * u * np.abs(D) + (e_p + e_m) * d
        sh = np.sin(D / 2)
        dsh = 0.5 * np.abs(np.cos(D / 2)) * dD + 2 * u * np.abs(sh)
        if same_lat:
            al = lat * d
            c = np.cos(al)
            dc = np.abs(np.sin(al)) * 2 * u * np.abs(al) + 2 * u * np.abs(c)
            s = np.abs(c * sh)
            ds = np.abs(sh) * dc + np.abs(c) * dsh + 3.5 * u * s
        else:
            s = np.abs(sh)
            ds = dsh + 2.5 * u * s
        a = np.arcsin(s)
        da = ds / np.sqrt(1 - s * s) + 2 * u * a
        return K * a, K * da + 5 * u * K * a

    ut, dut = speed(lon, True)
    vt, dvt = speed(lat, False)
    x = (lat - 35.0) / 10.0
    th = np.tanh(x)
    dth = (1 - th * th) * 3 * u * np.abs(x) + 2 * u * np.abs(th)
    g = 0.8 + 0.35 * (1 + th)
    dg = 0.35 * (dth + u * (1 + th)) + 2 * u * 0.35 * (1 + th) + 0.8 * u + u * g
    G = np.minimum(1.0, g)
    dG = np.where(g < 1 + dg, dg, 0.0)

    def inner(tr, dtr, wa, wb):
        sh = wa - wb
        t2 = 0.1 * sh * v / 15.0
        dt2 = (0.1 * np.abs(v) / 15.0) * u * np.abs(sh) + 5 * u * np.abs(t2)
        return tr * dG + G * dtr + u * G * tr + dt2, t2

    dUi, t2u = inner(ut, dut, envw[:, 0], envw[:, 2])
    dVi, t2v = inner(vt, dvt, envw[:, 1], envw[:, 3])
    # |Ui| <= G ut + |t2|: the sign of ut does not matter to a bound
    dUi = dUi + u * (G * ut + np.abs(t2u))
    dVi = dVi + u * (G * vt + np.abs(t2v))
    # where |U| exceeds v / 2 by more than |dU|, min(|U|, v / 2) is v / 2 whatever U is: vmax = 1.5 v does not see dU at all
    Ui, Vi, _ = inner_wind(lon, lat, v, envw, dt_out)
    dU = np.hypot(dUi, dVi)
    dU = np.where(np.hypot(Ui, Vi) - dU > 0.5 * v, 0.0, dU)
    return dU + 10 * u * vmax_identity(lon, lat, v, envw, dt_out)


def vmax_in(R, lon, lat, v, envw, dt_out, earth_R=EARTH_R, defect=None, rel=0.0):
    """The device's formulation in dtype R, operation for operation (nothing fused: the library is built with -ffp-contract=off):
    k_emit's neighbours — lane +-1 of a 64-lane wave through the shuffles, which give lanes 0 and 63 their own sample (and the last
    sample the zero of an idle lane); lanes 0 / 63 then take their outside neighbour from the dense output, the ends extrapolate
    from the other neighbour — and vmax_at: the same-latitude and same-longitude haversines with radians first, Ui / |U| and
    Vi / |U| in place of the angle (|U| == 0: (0, 1)), np_min's NaN rule.  defect: one of DEFECTS; rel: the size of 'relative'."""
    assert defect is None or defect in DEFECTS
    R = np.dtype(R).type
    x = [np.asarray(a, np.float64).astype(R) for a in (lon, lat)]
    v = np.asarray(v, np.float64).astype(R)
    w = np.asarray(envw, np.float64).reshape(-1, 4).astype(R)
    n = len(v)
    if n == 1:
        return np.full(1, np.nan, R)
    i = np.arange(n)
    lane = i % WAVE
    fix_lo, fix_hi = (lane == 0) & (i > 0), (lane == WAVE - 1) & (i < n - 1)
    nb = []
    for y in x:
        pad = np.concatenate([y, np.zeros(1, R)])                   # the lane after the last valid one holds ye = 0
        lo = np.where(lane == 0, y, pad[i - 1])                     # __shfl_up / __shfl_down: an edge lane reads itself
        hi = np.where(lane == WAVE - 1, y, pad[i + 1])
        lo_shuffled = lo.copy()
        if defect not in ('shuffle_edges', 'neighbour_time'):
            # ('neighbour_time': the dense output of the neighbour's step at ts(i) IS sample i wherever both lie in one accepted step,
            # so on rows alone it shows as the same values as 'shuffle_edges', by another path)
            lo[fix_lo] = y[i[fix_lo] - 1]
            hi[fix_hi] = y[i[fix_hi] + 1]
        lo_in, hi_in = (lo_shuffled if defect == 'end_before_fixup' else lo).copy(), hi.copy()
        if defect == 'no_extrapolation':
            lo[0], hi[n - 1] = y[0], y[n - 1]
        else:
            lo[0] = R(2) * y[0] - hi_in[0]
            hi[n - 1] = R(2) * y[n - 1] - lo_in[n - 1]
        nb.append((lo, hi))
    (lom, lop), (lam, lap) = nb
    lon, lat = x
    d, r_km, two = R(np.pi / 180.0), R(earth_R / 1000.), R(2)
    with np.errstate(all='ignore'):
        def arc(aa):
            return r_km * (two * np.arcsin(np.sqrt(aa)))
        sb, c = np.sin((lom * d - lop * d) / two), np.cos(lat * d)
        dlon = R(0.5) * (np.sign(lop - lom) * arc(R(0.0) + c * c * (sb * sb)))
        sa = np.sin((lam * d - lap * d) / two)
        dlat = R(0.5) * (np.sign(lap - lam) * arc(sa * sa))
        ut, vt = dlon * R(1000.) / R(dt_out), dlat * R(1000.) / R(dt_out)
        G = np.fmin(R(1.), R(0.8) + R(0.35) * (R(1.) + np.tanh((lat - R(35.)) / R(10.))))
        us, vs = w[:, 0] - w[:, 2], w[:, 1] - w[:, 3]
        if defect == 'G_one':
            G = np.ones(n, R)
        if defect == 'shear_low_only':
            us, vs = w[:, 0], w[:, 1]
        if defect == 'shear_swapped':
            us, vs = vs, us
        Ui = G * ut + R(0.1) * us * v / R(15.)
        Vi = G * vt + R(0.1) * vs * v / R(15.)
        mag = np.sqrt(Ui * Ui + Vi * Vi)
        q = (v * R(0.50)) / mag
        fac = np.where(np.isnan(q), q, np.where(q < R(1.0), q, R(1.0)))
        msin = np.where(mag == 0, R(0.0), Ui / mag)
        mcos = np.where(mag == 0, R(1.0), Vi / mag)
        ug = v * msin + Ui * fac
        vg = v * mcos + Vi * fac
        vm = np.sqrt(ug * ug + vg * vg)
    assert vm.dtype == R
    if defect == 'relative':
        vm = (vm.astype(np.float64) * (1.0 + rel)).astype(R)
    return vm


def vmax_errors(R, got, lon, lat, v, envw, dt_out):
    """e [n] = |got - vmax_ref| / vmax_bound(R) on one storm's rows (n > 1)"""
    ref = vmax_ref(lon, lat, v, envw, dt_out)
    with np.errstate(all='ignore'):
        return np.abs(np.asarray(got, np.float64) - ref) / vmax_bound(R, lon, lat, v, envw, dt_out)


def sample_classes(n):
    """which of a storm's n samples are ends, wave-edge lanes and workgroup-edge threads of k_emit"""
    i = np.arange(n)
    return dict(end=(i == 0) | (i == n - 1), wave=np.isin(i % WAVE, (0, WAVE - 1)), block=np.isin(i % BLOCK, (0, BLOCK - 1)))


def accept_flags(R, v, vmax, n, status, grid, v_thresh, v_2d_thresh, vmax_thresh):
    """(is_tc, accepted) of one storm from its rows (util/compute.py:185-189, 205): is_tc as rk_steps_numpy.is_tc; accepted = is_tc
    and n > 1 and any(vmax >= R(vmax_thresh)), NaNs never counting.  Exact."""
    R = np.dtype(R).type
    n = int(n)
    if status == GATED or n == 0:
        return False, False
    v, vmax = np.asarray(v)[:n], np.asarray(vmax)[:n]
    assert v.dtype == R and vmax.dtype == R
    tc = rk.is_tc(v, grid, v_thresh, v_2d_thresh)
    with np.errstate(invalid='ignore'):
        hit = bool((vmax >= R(vmax_thresh)).any())
    return tc, bool(tc and n > 1 and hit)


def census(batches):
    """What test_emit asks of its batches.  batches: a list of dicts with n_valid, status, is_tc, accepted [k] and fac (a list of
    per-storm arrays, or None entries for storms without a vmax).  Returns the counts."""
    c = dict(n1=0, n2=0, w0=0, w1=0, w63=0, b01=0, accepted=0, tc_only=0, fac_lt1=0, fac_eq1=0)
    for b in batches:
        n = np.asarray(b['n_valid'])
        on = (np.asarray(b['status']) != GATED) & (n > 0)
        c['n1'] += int((on & (n == 1)).sum())
        c['n2'] += int((on & (n == 2)).sum())
        c['w0'] += int((on & (n % WAVE == 0)).sum())
        c['w1'] += int((on & (n > 1) & (n % WAVE == 1)).sum())
        c['w63'] += int((on & (n % WAVE == WAVE - 1)).sum())
        c['b01'] += int((on & (n > 1) & np.isin(n % BLOCK, (0, 1))).sum())
        c['accepted'] += int(np.asarray(b['accepted']).sum())
        c['tc_only'] += int((np.asarray(b['is_tc']) & ~np.asarray(b['accepted'])).sum())
        for f in b['fac']:
            if f is not None:
                c['fac_lt1'] += int((f < 1).sum())
                c['fac_eq1'] += int((f == 1).sum())
    return c


# at least this many of each class (the issue's list)
CENSUS_MIN = dict(n1=2, n2=2, w0=2, w1=2, w63=2, b01=2, accepted=10, tc_only=10, fac_lt1=5000, fac_eq1=5000)
