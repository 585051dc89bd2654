"""NumPy restatement of the lookups of one RHS evaluation as the kernels spell them (csrc/tcr_device.h: locate_t, blend / blend4,
StaticLookup; csrc/tcr_stage.hip: axis_of<float>, axis_is_affine, k_to_f32), in ONE floating type throughout and without fused
operations: dtype=np.float32 is what the fp32 variant computes (tests/test_rhs_f32.py compares it bit for bit with
tcr_probe_rhs_f32_host's aux), dtype=np.float64 is the same code in the reference's precision — used only to show, without a GPU,
that the restatement equals the C oracle's bilinear (FITPACK's fpbisp / fpbspl with kx = ky = 1) bit for bit.

Every array below has the dtype R; integers are converted with astype(R) before they meet one, so that NumPy never promotes.
"""
import numpy as np

from oracle.scipy_port import BASIN_BOUNDS, crop_to_box


class Axis:
    """One axis as axis_of<R> forms it: knots rounded to R, dx = x[1] - x[0], rdx = 1 / dx, inv_step = (n - 1) / (xn - x0),
    per-cell reciprocal widths, and the affine test (x0 + i dx reproduces every knot, every 1 / (x[i+1] - x[i]) == rdx) in R."""

    def __init__(self, x, R):
        x = np.asarray(x, dtype=np.float64).astype(R)
        assert (x[1:] > x[:-1]).all()
        self.R, self.x, self.n = R, x, x.size
        self.x0, self.xn = x[0], x[-1]
        self.dx = x[1] - x[0]
        self.rdx = R(1.0) / self.dx
        self.inv_step = R(self.n - 1) / (x[-1] - x[0])
        self.rx = R(1.0) / (x[1:] - x[:-1])
        i = np.arange(self.n).astype(R)
        self.affine = bool((self.x0 + i * self.dx == x).all() and (self.rx == self.rdx).all())


def locate(A, arg, affine):
    """locate_t<R, AFFINE>: clamp, cell guess from inv_step, one step up / down (affine) or the knot walk (general), then
    w0 = 0 + f (xr - arg), w1 = f (arg - xl).  Returns (i, w0, w1)."""
    R = A.R
    arg = np.asarray(arg, dtype=np.float64).astype(R)
    arg = np.where(arg < A.x0, A.x0, arg)
    arg = np.where(arg > A.xn, A.xn, arg)
    n = A.n
    with np.errstate(invalid='ignore'):
        g = (arg - A.x0) * A.inv_step
        i = np.where(np.isnan(g), 0, g).astype(np.int64)       # (int) truncates; a NaN converts to 0 on the device
    i = np.clip(i, 0, n - 2)
    if affine:
        xl = A.x0 + i.astype(R) * A.dx
        xr = A.x0 + (i + 1).astype(R) * A.dx
        up = (i < n - 2) & (arg >= xr)
        dn = ~up & (i > 0) & (arg < xl)
        i = i + np.where(up, 1, np.where(dn, -1, 0))
        xl2 = np.where(up, xr, np.where(dn, A.x0 + i.astype(R) * A.dx, xl))
        xr2 = np.where(up, A.x0 + (i + 1).astype(R) * A.dx, np.where(dn, xl, xr))
        f = A.rdx
    else:
        while True:
            up = (i < n - 2) & (arg >= A.x[i + 1])
            if not up.any():
                break
            i = i + up
        while True:
            dn = (i > 0) & (arg < A.x[i])
            if not dn.any():
                break
            i = i - dn
        xl2, xr2, f = A.x[i], A.x[i + 1], A.rx[i]
    w0 = R(0.0) + f * (xr2 - arg)
    w1 = f * (arg - xl2)
    assert w0.dtype == R and w1.dtype == R
    return i, w0, w1


def blend(plane, cx, cy):
    """blend / blend4: the four-term sum in fpbisp's order — (x0,y0), (x0,y1), (x1,y0), (x1,y1), each term (c hx) hy."""
    (ix, wx0, wx1), (iy, wy0, wy1) = cx, cy
    R = plane.dtype.type
    sp = np.zeros(ix.shape, dtype=R)
    sp = sp + plane[iy, ix] * wx0 * wy0
    sp = sp + plane[iy + 1, ix] * wx0 * wy1
    sp = sp + plane[iy, ix + 1] * wx1 * wy0
    sp = sp + plane[iy + 1, ix + 1] * wx1 * wy1
    assert sp.dtype == R
    return sp


class Lookups:
    """The 20 bilinear lookups of one (environment, basin, month) in the type R: planes cropped as the product and the oracle crop
    them (util/basins.py:57-75), wind NaN -> 0 (bam_track.py:72-74), everything rounded to R once (k_to_f32; the narrow static
    modes hold exact values, which round to the same R).  The kernels take the affine path only when EVERY axis of the context is
    affine in R (host_eval_k); `affine` says which path this restatement took."""

    def __init__(self, env, basin, month0, R, bounds=None):
        b = BASIN_BOUNDS[basin] if bounds is None else bounds
        self.R = R

        def crop(lon, lat, X, nan0=False):
            lo, la, Xb = crop_to_box(b, lon, lat, np.asarray(X))
            Xb = np.asarray(Xb, dtype=np.float64)
            return lo, la, (np.nan_to_num(Xb) if nan0 else Xb).astype(R)

        planes = [crop(env.wlon, env.wlat, env.wnd_mean[month0, k], True) for k in range(4)]
        planes += [crop(env.wlon, env.wlat, env.wnd_cov[month0, k], True) for k in range(10)]
        self.wind = [p[2] for p in planes]
        self.wx, self.wy = Axis(planes[0][0], R), Axis(planes[0][1], R)
        th = [crop(env.lon, env.lat, getattr(env, name)[month0]) for name in ('vpot', 'chi', 'mld', 'strat')]
        self.thermo = [p[2] for p in th]
        self.tx, self.ty = Axis(th[0][0], R), Axis(th[0][1], R)
        hl, ha, self.land = crop(env.hlon, env.hlat, env.land)
        self.hx, self.hy = Axis(hl, R), Axis(ha, R)
        blon, blat = getattr(env, 'blon', None), getattr(env, 'blat', None)
        bl, ba, self.bathy = crop(env.hlon if blon is None else blon, env.hlat if blat is None else blat, env.bathy)
        self.bx, self.by = Axis(bl, R), Axis(ba, R)
        self.axes = dict(w=(self.wx, self.wy), t=(self.tx, self.ty), h=(self.hx, self.hy), b=(self.bx, self.by))
        self.affine = all(a.affine for pair in self.axes.values() for a in pair)

    def cells(self, which, lon, lat):
        ax, ay = self.axes[which]
        return locate(ax, lon, self.affine), locate(ay, lat, self.affine)

    def __call__(self, lon, lat):
        """[n, 20] in R: the 14 wind lookups (4 means, 10 packed covariances), vpot, chi, mld, strat, land, bathymetry — the
        layout of aux[:, :20] of tcr_probe_rhs_f32_host."""
        out = np.empty((len(lon), 20), dtype=self.R)
        cx, cy = self.cells('w', lon, lat)
        for k in range(14):
            out[:, k] = blend(self.wind[k], cx, cy)
        cx, cy = self.cells('t', lon, lat)
        for k in range(4):
            out[:, 14 + k] = blend(self.thermo[k], cx, cy)
        cx, cy = self.cells('h', lon, lat)
        out[:, 18] = blend(self.land, cx, cy)
        cx, cy = self.cells('b', lon, lat)
        out[:, 19] = blend(self.bathy, cx, cy)
        return out


def axis_points(x, R, rng, n_random):
    """The points of one axis the lookups are pinned at, as (class, value) in float64 holding R values (so that the device's
    rounding of them is the identity): below x0 and above xn (clamped), exactly x0 and xn, every knot of the first three and last
    three cells with its R neighbours one ulp below and above, every cell midpoint of those and a sample of the others, and
    n_random uniform points.  Classes: 0 clamped, 1 end knots, 2 knots and their neighbours, 3 midpoints, 4 random."""
    x = np.asarray(x, dtype=np.float64).astype(R)
    n = x.size
    span = R(x[-1] - x[0])
    pts = [(0, x[0] - R(0.37) * span / R(n)), (0, x[-1] + R(0.41) * span / R(n)), (0, x[0] - R(3.0)), (0, x[-1] + R(3.0)),
           (1, x[0]), (1, x[-1])]
    edge = sorted(set(list(range(0, min(4, n))) + list(range(max(0, n - 4), n))))
    for i in edge:
        pts += [(2, x[i]), (2, np.nextafter(x[i], R(-np.inf))), (2, np.nextafter(x[i], R(np.inf)))]
    mids = sorted(set(list(range(0, min(3, n - 1))) + list(range(max(0, n - 4), n - 1)) + list(range(0, n - 1, max(1, (n - 1) // 40)))))
    for i in mids:
        pts.append((3, R(0.5) * (x[i] + x[i + 1])))
    for v in rng.uniform(float(x[0]), float(x[-1]), n_random):
        pts.append((4, R(v)))
    cls = np.array([c for c, _ in pts])
    val = np.array([float(R(v)) for _, v in pts])
    return cls, val


def paired_points(xlon, xlat, R, seed, n_random=2000):
    """Longitudes and latitudes of axis_points paired so that every class of the one axis meets every class of the other, and
    every special point of either axis at least once; the random points pair off one to one."""
    rng = np.random.default_rng(seed)
    cx, vx = axis_points(xlon, R, rng, n_random)
    cy, vy = axis_points(xlat, R, rng, n_random)
    sx, sy = np.flatnonzero(cx < 4), np.flatnonzero(cy < 4)
    lon, lat = [vx[cx == 4]], [vy[cy == 4]]
    # every special x with a latitude of each class (cycling through that class's members), and the other way round
    for c in range(5):
        my = np.flatnonzero(cy == c)
        lon.append(vx[sx]); lat.append(vy[my[(np.arange(sx.size) * 7 + c) % my.size]])
        mx = np.flatnonzero(cx == c)
        lat.append(vy[sy]); lon.append(vx[mx[(np.arange(sy.size) * 5 + c) % mx.size]])
    return np.concatenate(lon), np.concatenate(lat)


# ---------------------------------------------------------------------------------------------------------------------------
# Part C of tests/test_rhs_f32.py: the continuous RHS of the fp32 variant against the fp64 C oracle on the SAME float-rounded
# data, so that only the arithmetic inside the RHS differs.  Outputs, in this order everywhere below:
OUTPUTS = ('dlon', 'dlat', 'dv', 'dm', 'envw0', 'envw1', 'envw2', 'envw3', 'alpha')
EARTH_R = 6.3781e6
EPS32 = 2.0 ** -24


def f32(x):
    """Round to float32, keep as float64 (what the fp32 variant stages of a double)."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def env_f32(env):
    """A copy of the environment with every floating array and axis put through float32."""
    import dataclasses
    over = {}
    for f in dataclasses.fields(env):
        x = getattr(env, f.name)
        if isinstance(x, np.ndarray) and x.dtype.kind == 'f':
            over[f.name] = f32(x)
    return dataclasses.replace(env, **over)


def params_f32(prm):
    import dataclasses
    over = {}
    for k in ('Ck', 'epsilon', 'kappa', 'u_beta', 'v_beta'):
        over[k] = float(f32(getattr(prm, k)))
    for k in ('y_alpha', 'm_alpha', 'alpha_max', 'alpha_min', 'steering_coefs'):
        over[k] = tuple(float(f32(x)) for x in getattr(prm, k))
    return dataclasses.replace(prm, **over)


def oracle_outputs(cme, prm, Fs, h_bl, t, lon, lat, v, m):
    """[n, 9] of the C oracle (OUTPUTS)."""
    from oracle import c_oracle
    d, w, a = c_oracle.rhs_points(cme, Fs, h_bl, t, lon, lat, v, m, prm=prm)
    return np.concatenate([d, w, a[:, None]], axis=1)


def cholesky_packed(cov):
    """LAPACK dpotrf('L') on the packed lower triangles cov [n, 10] (a00 a10 a11 a20 a21 a22 a30 a31 a32 a33) in float64:
    the factor [n, 4, 4] and, per pivot, ajj / a_jj (how much of the diagonal entry the subtraction leaves)."""
    n = cov.shape[0]
    a = np.zeros((n, 4, 4))
    k = 0
    for i in range(4):
        for j in range(i + 1):
            a[:, i, j] = cov[:, k]; k += 1
    Lc = np.zeros((n, 4, 4))
    piv = np.zeros((n, 4))
    with np.errstate(invalid='ignore', divide='ignore'):
        for j in range(4):
            ajj = a[:, j, j] - (Lc[:, j, :j] ** 2).sum(axis=1)
            piv[:, j] = ajj / a[:, j, j]
            Lc[:, j, j] = np.sqrt(ajj)
            for i in range(j + 1, 4):
                Lc[:, i, j] = (a[:, i, j] - (Lc[:, i, :j] * Lc[:, j, :j]).sum(axis=1)) / Lc[:, j, j]
    return Lc, piv


def select_continuous(L64, lon, lat):
    """The points at which no decision of the RHS can fall differently in the two precisions (L64: Lookups(env32, ..., float64),
    i.e. the oracle's own lookups on the float-rounded data): sea with all four land corners 0 (the land sum is exactly 0 in both),
    bathymetry < 0 and -mld > bathymetry + 1 m and strat != 0 (the mixing branch, clearly), PI != 0, and every fp64 Cholesky pivot above
    1e-3 of its diagonal entry."""
    q = L64(lon, lat).astype(np.float64)
    (ix, _, _), (iy, _, _) = L64.cells('h', lon, lat)
    P = L64.land
    sea = (P[iy, ix] == 0) & (P[iy + 1, ix] == 0) & (P[iy, ix + 1] == 0) & (P[iy + 1, ix + 1] == 0)
    mix = (q[:, 19] < 0) & (-q[:, 16] > q[:, 19] + 1.0) & (q[:, 17] != 0)
    _, piv = cholesky_packed(q[:, 4:14])
    with np.errstate(invalid='ignore'):
        pd = (piv > 1e-3).all(axis=1)
    return sea & mix & pd & (q[:, 14] != 0), dict(sea=sea, mix=mix, pd=pd)


def magnitudes(L64, prm, Fs, h_bl, t, lon, lat, v, m, ref):
    """mag [n, 9]: for each output the sum of the absolute values of the additive terms it is formed from, in float64 from the
    oracle's own values (ref = oracle_outputs, L64 = its lookups).  A quantity that is itself such a sum enters a later
    expression with its magnitude in place of its value:
      envw_i  = mu_i + sum_j L_ij F_j                         mag_w_i  = |mu_i| + sum_j |L_ij F_j|
      vb0     = (w0 c0 + w2 c1) + u_beta cos(lat)             mag_vb0  = mag_w0 |c0| + mag_w2 |c1| + |u_beta| cos(lat)
      vb1     = (w1 c0 + w3 c1) + sgn(lat) v_beta cos(lat)    mag_vb1  = mag_w1 |c0| + mag_w3 |c1| + |v_beta| cos(lat)
      dlon    = vb0 (180 / pi R) / cos(lat)                   mag_dlon = mag_vb0 (180 / pi R) / cos(lat)
      dlat    = vb1 (180 / pi R)                              mag_dlat = mag_vb1 (180 / pi R)
      alpha   = 1 - 0.87 exp(-z),  z = 0.01 strat^-0.4 mld uT PI / v, uT = |vb|
                                                              mag_al   = 1 + 0.87 exp(-z) (1 + z |mag_vb| / uT)
      dv      = ck_h (alpha beta PI^2 m^3 - (1 - gamma m^3) v^2), gamma = eps + alpha kappa
                                                              mag_dv   = ck_h (mag_al beta PI^2 m^3 + v^2 + (eps + mag_al kappa) m^3 v^2)
      dm      = ck_h ((1 - m) v - S chi m), S = |(w0 - w2, w1 - w3)|
                                                              mag_dm   = ck_h (v + m v + |(mag_w0 + mag_w2, mag_w1 + mag_w3)| chi m)"""
    q = L64(lon, lat).astype(np.float64)
    Lc, _ = cholesky_packed(q[:, 4:14])
    t_s = np.linspace(0, prm.total_time, prm.n_steps)
    F = np.stack([np.interp(t, t_s, Fs[k]) for k in range(4)], axis=1)
    mag = np.empty((len(t), 9))
    mag_w = np.abs(q[:, :4]) + np.abs(Lc * F[:, None, :]).sum(axis=2)
    mag[:, 4:8] = mag_w
    a = [np.clip((v * 1.94384) * prm.m_alpha[k] + prm.y_alpha[k], prm.alpha_min[k], prm.alpha_max[k]) for k in range(2)]
    c0, c1 = (a[0], a[1]) if prm.coupled_track else (np.full_like(v, prm.steering_coefs[0]), np.full_like(v, prm.steering_coefs[1]))
    cl = np.cos(lat * (np.pi / 180.0))
    deg = 1.0 / EARTH_R * 180.0 / np.pi
    w = ref[:, 4:8]
    vb0 = (w[:, 0] * c0 + w[:, 2] * c1) + prm.u_beta * cl
    vb1 = (w[:, 1] * c0 + w[:, 3] * c1) + (np.sign(lat) * prm.v_beta) * cl
    mag_vb0 = mag_w[:, 0] * np.abs(c0) + mag_w[:, 2] * np.abs(c1) + abs(prm.u_beta) * cl
    mag_vb1 = mag_w[:, 1] * np.abs(c0) + mag_w[:, 3] * np.abs(c1) + abs(prm.v_beta) * cl
    mag[:, 0] = mag_vb0 * deg / cl
    mag[:, 1] = mag_vb1 * deg
    vp, chi, h_m, gam = q[:, 14], q[:, 15], q[:, 16], q[:, 17]
    uT = np.hypot(vb0, vb1)
    with np.errstate(invalid='ignore', divide='ignore'):
        z = np.clip(0.01 * gam ** -0.4 * h_m * uT * vp / v, 0.0, 100.0)
        mag_al = 1.0 + 0.87 * np.exp(-z) * (1.0 + z * np.hypot(mag_vb0, mag_vb1) / uT)
    mag[:, 8] = mag_al
    ck_h = 0.5 * prm.Ck / h_bl
    m3 = m ** 3
    mag[:, 2] = ck_h * (mag_al * prm.beta * vp ** 2 * m3 + v ** 2 + (prm.epsilon + mag_al * prm.kappa) * m3 * v ** 2)
    mag[:, 3] = ck_h * (v + m * v + np.hypot(mag_w[:, 0] + mag_w[:, 2], mag_w[:, 1] + mag_w[:, 3]) * chi * m)
    return mag


def twin_response(cme, prm, Fs, h_bl, t, lon, lat, v, m, ref):
    """twin [n, 9]: the oracle's own response to one float32 ulp in each of lon, lat, v, m, up and down — per output the
    maximum of |ref_twin - ref| over the eight (in the manner of c_oracle.replayer's twin_storms)."""
    base = dict(lon=lon, lat=lat, v=v, m=m)
    twin = np.zeros_like(ref)
    for key in base:
        for sgn in (np.inf, -np.inf):
            pert = dict(base)
            pert[key] = np.nextafter(base[key].astype(np.float32), np.float32(sgn)).astype(np.float64)
            twin = np.fmax(twin, np.abs(oracle_outputs(cme, prm, Fs, h_bl, t, pert['lon'], pert['lat'], pert['v'], pert['m']) - ref))
    return twin


def normalised_error(got, ref, twin, mag):
    """|got - ref| / (twin + 2^-24 mag), [n, 9]"""
    return np.abs(got - ref) / (twin + EPS32 * mag)
