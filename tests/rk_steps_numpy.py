"""One RK45 step restated in NumPy, for tests/test_rk_steps.py: everything an accepted-step record (t_old, h, t_new, y_old[4], K[7][4])
says about the step that left it, recomputed from the record alone.

Written from SciPy — scipy/integrate/_ivp/rk.py (rk_step :14-70, _step_impl :113-171, _estimate_error_norm :173-177,
_dense_output_impl :179-181, RK45's tableau :384-420, RkDenseOutput._call_impl :552-574), common.py (select_initial_step :68-134, norm
:63-65) and ivp.py (t_eval emission :706-723) — in the type R of the run (np.float32 or np.float64): state, stage derivatives and the
tableau entries that multiply them are R, times and the step-size controller are float64, as the integrator's header states.  A
multiply-add that the integrator's compiler may or may not have fused exists here in both forms.

All functions work on arrays of records (leading axis = record)."""
from fractions import Fraction as Fr

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, 'np.longdouble must be the 80-bit x87 type: products of two doubles-from-floats must be exact'

# ---- Dormand-Prince, as exact fractions (rk.py:384-420)
C_FR = [Fr(0), Fr(1, 5), Fr(3, 10), Fr(4, 5), Fr(8, 9), Fr(1), Fr(1)]
A_FR = [[],
        [Fr(1, 5)],
        [Fr(3, 40), Fr(9, 40)],
        [Fr(44, 45), Fr(-56, 15), Fr(32, 9)],
        [Fr(19372, 6561), Fr(-25360, 2187), Fr(64448, 6561), Fr(-212, 729)],
        [Fr(9017, 3168), Fr(-355, 33), Fr(46732, 5247), Fr(49, 176), Fr(-5103, 18656)]]
B_FR = [Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84)]
E_FR = [Fr(-71, 57600), Fr(0), Fr(71, 16695), Fr(-71, 1920), Fr(17253, 339200), Fr(-22, 525), Fr(1, 40)]
P_FR = [[Fr(1), Fr(-8048581381, 2820520608), Fr(8663915743, 2820520608), Fr(-12715105075, 11282082432)],
        [Fr(0)] * 4,
        [Fr(0), Fr(131558114200, 32700410799), Fr(-68118460800, 10900136933), Fr(87487479700, 32700410799)],
        [Fr(0), Fr(-1754552775, 470086768), Fr(14199869525, 1410260304), Fr(-10690763975, 1880347072)],
        [Fr(0), Fr(127303824393, 49829197408), Fr(-318862633887, 49829197408), Fr(701980252875, 199316789632)],
        [Fr(0), Fr(-282668133, 205662961), Fr(2019193451, 616988883), Fr(-1453857185, 822651844)],
        [Fr(0), Fr(40617522, 29380423), Fr(-110615467, 29380423), Fr(69997945, 29380423)]]


class Tableau:
    """The tableau as a run of type R holds it: every entry is the double nearest the fraction (float(Fraction) rounds
    correctly, as the division of two exactly represented integers does); A, B and P are then rounded to R, C and E stay double.
    The arrays are plain attributes so that a test can plant a defect in a copy (`planted`)."""

    def __init__(self, R):
        self.R = R
        self.A = np.zeros((6, 5), R)
        for s, row in enumerate(A_FR):
            for j, a in enumerate(row):
                self.A[s, j] = R(float(a))
        self.B = np.array([R(float(b)) for b in B_FR], R)
        self.C = np.array([float(c) for c in C_FR], np.float64)
        self.E = np.array([float(e) for e in E_FR], np.float64)
        self.P = np.array([[R(float(p)) for p in row] for row in P_FR], R)
        self.sc_with_max = True                 # rk.py:151: scale from max(|y|, |y_new|)

    def planted(self, what, idx, rel):
        """A copy with one entry multiplied by (1 + rel); what = 'A' | 'B' | 'C' | 'E' | 'P' (idx: the entry; for P a column:
        every entry of it) | 'sc' (|y| alone in the error scale; idx and rel unused)."""
        t = Tableau(self.R)
        if what == 'sc':
            t.sc_with_max = False
        elif what == 'P':
            t.P[:, idx] = (t.P[:, idx].astype(np.float64) * (1 + rel)).astype(self.R)
        else:
            a = getattr(t, what)
            a[idx] = a.dtype.type(float(a[idx]) * (1 + rel))
        return t


class Records:
    """Accepted-step records: t_old, h, t_new [N] float64; y [N, 4], K [N, 7, 4] in R."""

    def __init__(self, t_old, h, t_new, y, K):
        self.t_old, self.h, self.t_new = (np.ascontiguousarray(x, dtype=np.float64) for x in (t_old, h, t_new))
        self.y, self.K = np.ascontiguousarray(y), np.ascontiguousarray(K)
        assert self.y.dtype == self.K.dtype and self.y.dtype in (np.float32, np.float64)
        self.R = self.y.dtype.type

    def __len__(self):
        return len(self.h)

    def __getitem__(self, idx):
        return Records(self.t_old[idx], self.h[idx], self.t_new[idx], self.y[idx], self.K[idx])

    @staticmethod
    def concat(recs):
        return Records(*[np.concatenate([getattr(r, k) for r in recs]) for k in ('t_old', 'h', 't_new', 'y', 'K')])


def unit_roundoff(R):
    return 2.0 ** -24 if R == np.float32 else 2.0 ** -53


# ---- the fused multiply-add, a * b + c rounded once
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma(a, b, c, R):
    """a * b + c with ONE rounding to R.
    float32, exact: the product of two floats is exact in double; s = fl64(p + c) with its exact remainder e (TwoSum).  Rounding s
    to float is the rounding of p + c unless s lies exactly half way between two floats while e != 0 — every such tie point is a
    double, and p + c lies on s's side of every other one — and then e's sign decides.
    float64, exact: rational arithmetic element by element (a few microseconds each)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, R), np.asarray(b, R), np.asarray(c, R))
    if R == np.float32:
        p = a.astype(np.float64) * b.astype(np.float64)
        s, e = _two_sum(p, c.astype(np.float64))
        r = s.astype(np.float32)
        with np.errstate(invalid='ignore', over='ignore'):
            d = s - r.astype(np.float64)
            other = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)))
            tie = (d != 0) & (r.astype(np.float64) + other.astype(np.float64) == 2.0 * s) & (e != 0) & np.isfinite(s)
            # at a tie the exact sum s + e lies on e's side of s; `other` is the neighbour on d's side of r, r the one on the other side
            out = np.where(tie & (np.sign(e) == np.sign(d)), other, r)
        return out.astype(np.float32)
    return _fma64(a, b, c).astype(np.float64)


def _fma64_one(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fr(a) * Fr(b) + Fr(c))            # float(Fraction) rounds correctly


_fma64 = np.frompyfunc(_fma64_one, 3, 1)


def _mul_add(a, b, c, R, fused):
    """c + a * b in R: fused, or the product and the sum rounded separately; `fused` may be one flag per component (last axis),
    for a compiler that chose differently for different components"""
    if np.ndim(fused) == 0 and fused:
        return fma(a, b, c, R)
    plain = (np.asarray(c, R) + np.asarray(a, R) * np.asarray(b, R)).astype(R)
    if np.ndim(fused) == 0:
        return plain
    return np.where(np.asarray(fused, bool), fma(a, b, c, R), plain).astype(R)


# ---- stages and y_new (rk_step, rk.py:62-68)
def stage_input(rec, s, fused, tab=None, fused_last=None):
    """The point at which K[s] is evaluated, s = 1..5: y + (sum_{j<s} K_j a_sj) * h — the sum accumulated from zero with j
    ascending (np.dot(K[:s].T, a[:s]) for one component), then times R(h), plus y (rk.py:65-66).  [N, 4] in R."""
    R = rec.R
    tab = tab or Tableau(R)
    dy = np.zeros_like(rec.y)
    for j in range(s):
        dy = _mul_add(rec.K[:, j], tab.A[s, j], dy, R, fused)
    hR = rec.h.astype(R)[:, None]
    return _mul_add(dy, hR, rec.y, R, fused if fused_last is None else fused_last)


def stage_time(rec, s, tab=None, fused=False):
    """t + c_s h in float64 (rk.py:66); s = 6: t + h.  fused: as one multiply-add (times are float64 in either type of run)"""
    tab = tab or Tableau(rec.R)
    if fused:
        return fma(np.full(len(rec), tab.C[s]), rec.h, rec.t_old, np.float64)
    return rec.t_old + tab.C[s] * rec.h


def y_new_variant(rec, fused, tab=None, fused_last=None):
    """y + h * dot(K[:-1].T, B) (rk.py:68) in R, every multiply-add fused or none: [N, 4].  fused_last: the final y + h * dy
    fused or not on its own (the two mixed forms, for naming what a compiler emitted)."""
    R = rec.R
    tab = tab or Tableau(R)
    dy = np.zeros_like(rec.y)
    for j in range(6):
        dy = _mul_add(rec.K[:, j], tab.B[j], dy, R, fused)
    return _mul_add(rec.h.astype(R)[:, None], dy, rec.y, R, fused if fused_last is None else fused_last)


def y_new_ref(rec, tab=None):
    """y + R(h) * sum_j R(B_j) K_j in long double on the R values (each product of two R values is exact in it): [N, 4] longdouble"""
    tab = tab or Tableau(rec.R)
    acc = np.zeros(rec.y.shape, LD)
    for j in range(6):
        acc = acc + rec.K[:, j].astype(LD) * LD(tab.B[j])
    return rec.y.astype(LD) + rec.h.astype(rec.R).astype(LD)[:, None] * acc


def y_new_bound(rec, tab=None):
    """1.01 (u |y_new_ref| + 8 u |h| sum_j |B_j K_j|): six multiply-adds and the final one, each rounded once or twice — the
    forward error of the recursive sum (gamma_7 <= 8 u on the products' magnitudes, times |h|) plus the last rounding; it
    holds for every mixture of fused and separate operations."""
    R = rec.R
    tab = tab or Tableau(R)
    u = unit_roundoff(R)
    mag = np.zeros(rec.y.shape, np.float64)
    for j in range(6):
        mag += np.abs(rec.K[:, j].astype(np.float64) * float(tab.B[j]))
    return 1.01 * (u * np.abs(y_new_ref(rec, tab)).astype(np.float64) + 8 * u * np.abs(rec.h)[:, None] * mag)


# ---- error norm and controller (rk.py:147-165, 173-177)
def _scale(rec, y_new, rtol, atol, tab):
    y, yn = np.abs(rec.y.astype(np.float64)), np.abs(np.asarray(y_new, np.float64))
    return atol + (np.maximum(y, yn) if tab.sc_with_max else y) * rtol


def err(rec, y_new, rtol, atol, tab=None):
    """norm(dot(K.T, E) * h / scale), norm = 2-norm / sqrt(size), in long double from the R stage derivatives: [N] float64"""
    tab = tab or Tableau(rec.R)
    sc = _scale(rec, y_new, rtol, atol, tab)
    acc = np.zeros(rec.y.shape, LD)
    for j in range(7):
        acc = acc + rec.K[:, j].astype(LD) * LD(tab.E[j])
    e = acc * rec.h.astype(LD)[:, None] / sc.astype(LD)
    return (np.sqrt((e * e).sum(axis=1)) / LD(2)).astype(np.float64)


def err_abs_bound(rec, y_new, rtol, atol, tab=None):
    """How far a float64 evaluation of the error norm may lie from `err`: per component 8 2^-53 |h| sum_j |E_j K_j| / scale
    (seven multiply-adds, the product with h, the division), carried through the norm (| ||a + d|| - ||a|| | <= ||d||)."""
    tab = tab or Tableau(rec.R)
    sc = _scale(rec, y_new, rtol, atol, tab)
    mag = np.zeros(rec.y.shape, np.float64)
    for j in range(7):
        mag += np.abs(rec.K[:, j].astype(np.float64) * tab.E[j])
    d = 8 * 2.0 ** -53 * np.abs(rec.h)[:, None] * mag / sc
    return np.sqrt((d * d).sum(axis=1)) / 2.0


SAFETY, MIN_FACTOR, MAX_FACTOR = 0.9, 0.2, 10.0


def factor(e):
    """rk.py:157-161 with error_exponent = -1 / 5: the factor of an accepted step"""
    e = np.asarray(e, np.float64)
    with np.errstate(divide='ignore'):
        return np.where(e == 0, MAX_FACTOR, np.minimum(MAX_FACTOR, SAFETY * e ** -0.2))


def factor_interval(rec, y_new, rtol, atol, tab=None):
    """[lo, hi] that contains the factor of an accepted step as float64 code computes it: err^-0.2 from `err` moved by the
    first-order effect of err_abs_bound (d(err^-0.2) / err^-0.2 = -0.2 d(err) / err) and by 4 2^-53 relative for the power itself
    (2 ulp), then the float64 operations of rk.py:157-161, each monotone, on the two ends.  Also returns err and its bound."""
    e = err(rec, y_new, rtol, atol, tab)
    eb = err_abs_bound(rec, y_new, rtol, atol, tab)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        pw = e.astype(LD) ** LD(-0.2)
        delta = 0.2 * eb / e + 4 * 2.0 ** -53
        lo = np.nextafter((pw * (1 - delta)).astype(np.float64), -np.inf)
        hi = np.nextafter((pw * (1 + delta)).astype(np.float64), np.inf)
    f_lo = np.where(e == 0, MAX_FACTOR, np.minimum(MAX_FACTOR, SAFETY * lo))
    f_hi = np.where(e == 0, MAX_FACTOR, np.minimum(MAX_FACTOR, SAFETY * hi))
    return f_lo, f_hi, e, eb


def clipped_step(t, h_abs, t_bound, max_step):
    """The h a step from t with the proposed |h| = h_abs records (rk.py:127-146): clamp to max_step, t_new = t + h, clip to
    t_bound, h = t_new - t — two float64 roundings that the recorded h carries.  Monotone in h_abs.  Returns (h, t_new)."""
    ha = np.minimum(np.asarray(h_abs, np.float64), max_step)
    t_new = t + ha
    t_new = np.where(t_new - t_bound > 0, t_bound, t_new)
    return t_new - t, t_new


# ---- the first step (common.py:68-134)
def _norm(x):
    return np.sqrt((x * x).sum(axis=-1)) / np.sqrt(x.shape[-1])


def initial_h0(y0, f0, rtol, atol, t_bound):
    """h0 of select_initial_step (common.py:112-121) from R arrays [N, 4]: float64 [N]"""
    sc = atol + np.abs(y0.astype(np.float64)) * rtol
    d0, d1 = _norm(y0.astype(np.float64) / sc), _norm(f0.astype(np.float64) / sc)
    with np.errstate(divide='ignore', invalid='ignore'):
        h0 = np.where((d0 < 1e-5) | (d1 < 1e-5), 1e-6, 0.01 * d0 / d1)
    return np.minimum(h0, t_bound)


def initial_y1(y0, f0, h0, fused):
    """y0 + h0 * direction * f0 (common.py:122) in R: (R(h0) * 1) * f0 + y0"""
    R = y0.dtype.type
    hR = (np.asarray(h0).astype(R) * R(1.0))[:, None]
    return _mul_add(hR, f0, y0, R, fused)


def initial_h(y0, f0, f1, h0, rtol, atol, t_bound, max_step):
    """select_initial_step's result (common.py:124-134) with order = 4; f1 - f0 is formed in R like every state-typed array"""
    sc = atol + np.abs(y0.astype(np.float64)) * rtol
    d1 = _norm(f0.astype(np.float64) / sc)
    d2 = _norm((f1 - f0).astype(np.float64) / sc) / h0
    with np.errstate(divide='ignore'):
        h1 = np.where((d1 <= 1e-15) & (d2 <= 1e-15), np.maximum(1e-6, h0 * 1e-3), (0.01 / np.maximum(d1, d2)) ** 0.2)
    return np.minimum(np.minimum(100 * h0, h1), min(t_bound, max_step))


# ---- the output grid (ivp.py:706-723 on t_eval = np.linspace(0, total_time, n_steps))
class Grid:
    def __init__(self, total_time, n_steps):
        self.ts = np.linspace(0, total_time, n_steps)
        self.total_time, self.n_steps = float(total_time), int(n_steps)

    def samples_upto(self, t):
        """number of samples <= t: np.searchsorted(t_eval, t, side='right')"""
        return np.searchsorted(self.ts, t, side='right')

    def ts_at(self, i):
        return self.ts[i]


# ---- dense output (rk.py:179-181, 552-574)
def dense_rows(rec, tab=None):
    """Q[c][k] = sum_q K[q][c] R(P[q][k]) (K.T.dot(P)), accumulated from zero with q ascending, every operation rounded to R:
    [N, 4 (c), 4 (k)]"""
    R = rec.R
    tab = tab or Tableau(R)
    Q = np.zeros((len(rec), 4, 4), R)
    for k in range(4):
        acc = np.zeros((len(rec), 4), R)
        for q in range(7):
            acc = (acc + (rec.K[:, q] * tab.P[q, k]).astype(R)).astype(R)
        Q[:, :, k] = acc
    return Q


def dense_eval(rec, Q, idx, t, powers=(1, 2, 3, 4)):
    """y_old + h * Q . (x, x^2, x^3, x^4) of records idx at times t (rk.py:552-574): x = R((t - t_old) / h) with the division in
    float64, powers by repeated multiplication, the four terms added in order, then R(h) * acc + y_old; nothing fused.
    `powers`: the power of x each column of Q meets (a test plants a wrong one).  [len(idx), 4] in R"""
    R = rec.R
    x = ((t - rec.t_old[idx]) / rec.h[idx]).astype(R)
    p = [x]
    for _ in range(max(powers) - 1):
        p.append((p[-1] * x).astype(R))
    acc = np.zeros((len(idx), 4), R)
    for k in range(4):
        acc = (acc + (Q[idx, :, k] * p[powers[k] - 1][:, None]).astype(R)).astype(R)
    return ((rec.h[idx].astype(R)[:, None] * acc).astype(R) + rec.y[idx]).astype(R)


def storm_rows(rec, grid, n_valid, tab=None):
    """The rows [n_valid, 4] one storm's records emit: record j owns the samples [samples_upto(t_old) (0 for j = 0),
    samples_upto(t_new)), cut at n_valid (ivp.py:706-723).  Returns (rows, owner) — owner[i] the record of sample i, -1 if none."""
    Q = dense_rows(rec, tab)
    lo = grid.samples_upto(rec.t_old)
    if len(rec):
        lo[0] = 0
    hi = np.minimum(grid.samples_upto(rec.t_new), n_valid)
    owner = np.full(n_valid, -1, np.int64)
    for j in range(len(rec)):
        owner[lo[j]:hi[j]] = j
    rows = np.full((n_valid, 4), np.nan, rec.R)
    ok = owner >= 0
    if ok.any():
        rows[ok] = dense_eval(rec, Q, owner[ok], grid.ts[:n_valid][ok])
    return rows, owner


# ---- accept test 1 (util/compute.py:185-189)
def v2d(v_row, grid, t2d=2 * 86400.0):
    """np.interp(2 d, res.t, v) on the emitted samples v_row [n_valid]: the float64 expression on widened values, clamped to the
    last sample"""
    n = len(v_row)
    if t2d >= grid.ts[n - 1]:
        return float(v_row[n - 1])
    j = int(np.floor(t2d / (grid.total_time / (grid.n_steps - 1))))
    lo, hi = float(v_row[j]), float(v_row[j + 1])
    return (hi - lo) / (grid.ts[j + 1] - grid.ts[j]) * (t2d - grid.ts[j]) + lo


def is_tc(v_row, grid, v_thresh, v_2d_thresh):
    return bool(len(v_row) > 0 and (v_row.astype(np.float64) >= v_thresh).any() and v2d(v_row, grid) >= v_2d_thresh)


# ---- a stepper built from the pieces above (the CPU tests: against scipy.integrate.RK45, and as the source of synthetic records)
def step(fun, t, y, f, h_abs, t_bound, R, fused, rtol, atol, max_step, tab=None):
    """_step_impl (rk.py:113-171): attempts from (t, y, f = fun(t, y)) with the proposal h_abs until one is accepted.  Returns
    (record of the accepted attempt or None if the step size underflowed, y_new, the next proposal, [(accepted, t, h)] of the attempts)."""
    tab = tab or Tableau(R)
    log, rejected = [], False
    min_step = 10 * abs(np.nextafter(t, np.inf) - t)
    h_abs = max_step if h_abs > max_step else (min_step if h_abs < min_step else h_abs)
    while True:
        if h_abs < min_step:
            return None, None, h_abs, log
        h, t_new = (float(x) for x in clipped_step(t, h_abs, t_bound, max_step))
        h_abs = abs(h)
        K = np.zeros((1, 7, 4), R)
        K[0, 0] = f
        one = Records([t], [h], [t_new], np.asarray(y, R)[None], K)
        for s in range(1, 6):
            one.K[0, s] = fun(float(stage_time(one, s, tab)[0]), stage_input(one, s, fused, tab)[0])
        yn = y_new_variant(one, fused, tab)[0]
        one.K[0, 6] = fun(t + h, yn)
        e = float(err(one, yn[None], rtol, atol, tab)[0])
        if e < 1:
            fac = float(factor(e))
            if rejected:
                fac = min(1.0, fac)
            log.append((True, t, h))
            return one, yn, h_abs * fac, log
        log.append((False, t, h))
        h_abs *= max(MIN_FACTOR, SAFETY * e ** -0.2)
        rejected = True


def first_step(fun, y0, t_bound, R, fused, rtol, atol, max_step):
    """RungeKutta.__init__ (rk.py:93-105): f0 and select_initial_step.  Returns (f0, h_abs, h0, y1, f1)."""
    y = np.asarray(y0, R)
    f = np.asarray(fun(0.0, y), R)
    h0 = initial_h0(y[None], f[None], rtol, atol, t_bound)
    y1 = initial_y1(y[None], f[None], h0, fused)[0]
    f1 = np.asarray(fun(float(h0[0]), y1), R)
    return f, float(initial_h(y[None], f[None], f1[None], h0, rtol, atol, t_bound, max_step)[0]), float(h0[0]), y1, f1


def run(fun, y0, t_bound, R, fused, rtol, atol, max_step, tab=None, max_accept=64, stop=None):
    """RK45 from t = 0 with the pieces above, one system: fun(t, y[4] in R) -> [4] in R.  Returns a dict: 'rec' (Records of the
    accepted steps), 'log' [(accepted, t, h)] of every attempt, 'status' ('finished' | 'stopped' | 'max_accept' | 'failed'),
    'y_end'.  stop(t, y) -> True ends the run after an accepted step (a terminal event at the step's end)."""
    y = np.asarray(y0, R)
    t = 0.0
    f, h_abs, _, _, _ = first_step(fun, y, t_bound, R, fused, rtol, atol, max_step)
    recs, log, status = [], [], 'max_accept'
    while len(recs) < max_accept:
        one, yn, h_abs, lg = step(fun, t, y, f, h_abs, t_bound, R, fused, rtol, atol, max_step, tab)
        log += lg
        if one is None:
            status = 'failed'
            break
        recs.append(one)
        t, y, f = float(one.t_new[0]), yn, one.K[0, 6].copy()
        if t - t_bound >= 0:
            status = 'finished'
            break
        if stop is not None and stop(t, y):
            status = 'stopped'
            break
    rec = Records.concat(recs) if recs else Records(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 4), R), np.zeros((0, 7, 4), R))
    return dict(rec=rec, log=log, status=status, y_end=y, t_end=t)
