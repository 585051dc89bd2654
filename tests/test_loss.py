"""Portfolio loss (tropical_cyclone_risk_amd/loss.py, csrc/tcr_loss.hip): the Emanuel (2011) damage function on the wind
footprint, summed over the sites inside the footprint scan.  CPU tests pin the damage function, the loss curves, the argument
handling, the CLI and the C struct layout; GPU tests (`-m gpu`) check the fused sums against NumPy sums over the existing
footprint entry point's site_max, against the footprint's NumPy restatement, and their bit identity."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import loss_numpy as LN
from tests import windfield_numpy as WN
from tests import test_windfield as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 3600.0
U = LN.U                                                                    # 2^-52


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_damage_function_by_hand():
    from tropical_cyclone_risk_amd import loss
    for D in (loss.damage, LN.damage):
        assert float(D(25.7, 25.7, 74.7)) == 0.0
        assert float(D(74.7, 25.7, 74.7)) == 0.5
        assert float(D(10.0, 25.7, 74.7)) == 0.0 and float(D(0.0, 25.7, 74.7)) == 0.0 and float(D(np.nan, 25.7, 74.7)) == 0.0
        # x = 2: 8 / 9; x = 1/2: 1 / 9
        assert math.isclose(float(D(25.7 + 2 * 49.0, 25.7, 74.7)), 8.0 / 9.0, rel_tol=1e-14)
        assert math.isclose(float(D(20.0 + 15.0, 20.0, 50.0)), 1.0 / 9.0, rel_tol=1e-14)
        m = np.linspace(0.0, 400.0, 4001)
        d = D(m, 25.7, 74.7)
        assert (np.diff(d) >= 0).all() and (np.diff(d[m > 25.7]) > 0).all() and (d < 1).all() and (d >= 0).all()
        assert float(D(1e4, 25.7, 74.7)) > 1 - 1e-6 and float(D(1e7, 25.7, 74.7)) <= 1.0
        # one v_half per site
        assert np.array_equal(D(np.array([60.0, 60.0]), 20.0, np.array([60.0, 100.0])), [0.5, 1.0 / 9.0])
    assert loss.V_THRESH == 25.7 and loss.V_HALF == 74.7
    m = np.concatenate([np.linspace(0, 120, 500), [np.nan]])
    assert np.array_equal(loss.damage(m), LN.damage(m, 25.7, 74.7))


def test_loss_curve_and_average_annual_loss():
    from tropical_cyclone_risk_amd import loss
    y = [5.0, 0.0, 3.0, 9.0, 1.0]
    got = loss.loss_curve(y, 5, [5, 2.5, 2, 1, 10])
    assert np.array_equal(got[:4], [9.0, 5.0, 3.0, 0.0]) and np.isnan(got[4])
    # eight years, three of them without a loss on record: 9 5 3 1 0 0 0 0
    got = loss.loss_curve(y, 8, [8, 4, 3, 2, 1.6, 1, 8.5])
    assert np.array_equal(got[:6], [9.0, 5.0, 3.0, 1.0, 0.0, 0.0]) and np.isnan(got[6])
    rng = np.random.default_rng(3)
    for n, total in ((1, 1), (7, 7), (40, 45), (0, 3)):
        yl = rng.lognormal(0, 2, n)
        T = np.concatenate([rng.uniform(0.3, total + 2, 20), [1.0, total, total / 3.0, total / 7.0]])
        a, b = loss.loss_curve(yl, total, T), LN.loss_curve(yl, total, T)
        assert np.array_equal(a, b, equal_nan=True)
    assert loss.average_annual_loss(y, 5) == 3.6
    assert loss.average_annual_loss(np.array(y), 8) == 18.0 / 8.0
    for bad in (dict(total_years=4), dict(total_years=0), dict(return_periods=[0.0]), dict(return_periods=[np.nan])):
        with pytest.raises(ValueError):
            loss.loss_curve(**dict(dict(year_losses=y, total_years=5, return_periods=[2.0]), **bad))
    # consistent with hazard.return_periods: the loss at T is exceeded or equalled in total / T of the years
    from tropical_cyclone_risk_amd import hazard
    counts = np.array([[(np.array(y) >= 3.0).sum()]])
    assert loss.loss_curve(y, 5, hazard.return_periods(counts, 5).ravel())[0] == 3.0


def test_year_loss_table_with_empty_groups():
    from tropical_cyclone_risk_amd import loss
    e = np.array([4.0, 1.0, 0.0, 2.5, 7.0])
    g = np.array([2, 0, 2, 4, 2])
    agg, mx = loss.year_loss_table(e, g, 6)
    assert np.array_equal(agg, [1.0, 0.0, 11.0, 0.0, 2.5, 0.0]) and np.array_equal(mx, [1.0, 0.0, 7.0, 0.0, 2.5, 0.0])
    ra, rm, _ = LN.year_table(e, g, 6)
    assert np.array_equal(agg, ra) and np.array_equal(mx, rm)
    agg, mx = loss.year_loss_table(np.zeros(0), np.zeros(0, np.int64), 3)
    assert np.array_equal(agg, np.zeros(3)) and np.array_equal(mx, np.zeros(3))
    for bad in ((e, g, 4), (e, g[:4], 6), (e, -g, 6), (e, g.astype(float), 6)):
        with pytest.raises(ValueError):
            loss.year_loss_table(*bad)


def test_loss_struct_layout_matches_header():
    from tropical_cyclone_risk_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tcrisk_hip.h"\nint main(void){printf("%zu %zu %zu\\n",'
           'sizeof(tcr_loss_params),offsetof(tcr_loss_params, v_thresh),offsetof(tcr_loss_params, v_half));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'sz.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 'sz')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    P = _lib.LossParams
    assert sizes == [ctypes.sizeof(P), P.v_thresh.offset, P.v_half.offset]


def test_loss_symbols_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_loss_dev', 'tcr_loss_host'):
        assert hasattr(L, name), name


def test_argument_errors_before_any_device_work():
    from tropical_cyclone_risk_amd import loss
    rng = np.random.default_rng(0)
    lon, lat, v = 280 + rng.random((3, 5)), 20 + rng.random((3, 5)), 30 + rng.random((3, 5))
    env = [np.zeros((3, 5))] * 4
    g = np.zeros(3, np.int64)
    base = dict(lon=lon, lat=lat, v=v, env=env, groups=g, site_lon=np.array([280.0, 281.0]), site_lat=np.array([20.0, 21.0]),
                value=np.array([1.0, 2.0]), dt_s=DT)
    bad = [dict(value=np.array([1.0, -2.0])), dict(value=np.array([np.nan, 2.0])), dict(value=np.array([1.0, np.inf])),
           dict(value=np.array([1.0, 2.0, 3.0])), dict(value=np.array([1.0])),
           dict(v_half=25.7), dict(v_half=20.0), dict(v_half=np.nan), dict(v_half=np.array([74.7, 25.7])),
           dict(v_half=np.array([74.7, np.nan])), dict(v_half=np.array([74.7, 80.0, 90.0])), dict(v_thresh=np.nan),
           dict(v_thresh=-1.0), dict(v_thresh=np.inf),
           # every windfield argument error still raises
           dict(r_out_km=0.0), dict(r_out_km=2000.5), dict(r_out_km=np.nan), dict(substeps=0), dict(substeps=65),
           dict(substeps=1.5), dict(ck_cd=0.0), dict(ck_cd=2.0), dict(dt_s=0.0), dict(dt_s=np.inf),
           dict(thresholds=np.array([20.0, 10.0])), dict(thresholds=np.arange(65.0)), dict(thresholds=np.array([])),
           dict(thresholds=np.array([10.0, np.inf])), dict(rmax_km=0.0), dict(rmax_km=-5.0), dict(rmax_km=np.full((3, 4), 20.0)),
           dict(rmax_km=np.where(np.arange(5) == 3, 0.0, 20.0) * np.ones((3, 1))), dict(env=env[:3]),
           dict(v=v[:, :4]), dict(groups=np.zeros(2, np.int64)), dict(groups=np.array([0, -1, 0])),
           dict(site_lat=np.array([np.nan, 1.0])), dict(site_lon=np.array([1.0, 2.0, 3.0])),
           dict(groups=np.array([0, 1, 2]), n_groups=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            loss.portfolio_loss(**dict(base, **kw))


def test_cli_arguments_and_exposure_file(tmp_path):
    from tropical_cyclone_risk_amd import loss
    a = loss.parse_args(['x.nc', 'y.nc', '--exposure', 'e.csv', '--v-thresh', '20', '--v-half', '60', '--rmax-km', '25',
                         '--r-out-km', '300', '--substeps', '4', '--ck-cd', '0.9', '--return-periods', '2,10,2.5', '--out', 'o.npz'])
    assert a.tracks == ['x.nc', 'y.nc'] and a.exposure == 'e.csv' and a.v_thresh == 20.0 and a.v_half == 60.0
    assert a.rmax_km == 25.0 and a.r_out_km == 300.0 and a.substeps == 4 and a.ck_cd == 0.9 and a.out == 'o.npz'
    assert np.array_equal(a.return_periods, [2.0, 10.0, 2.5])
    b = loss.parse_args(['x.nc', '--exposure', 'e.csv'])
    assert b.v_thresh == 25.7 and b.v_half == 74.7 and b.rmax_km is None and b.ck_cd is None and b.r_out_km == 500.0
    assert b.substeps == 1 and b.out == 'loss.npz' and np.array_equal(b.return_periods, [10, 25, 50, 100, 250])
    for bad in (['x.nc'], ['x.nc', '--exposure', 'e.csv', '--return-periods', '10,x'],
                ['x.nc', '--exposure', 'e.csv', '--return-periods', '0']):
        with pytest.raises(SystemExit):
            loss.parse_args(bad)
    fn = tmp_path / 'e.csv'
    fn.write_text('lon,lat,value,v_half\n-80.19,25.76,1.5e6\n279.5;26.0;2e6;60.5\n# a comment\n1,2\n-75.0,35.2,0,\n3,4,abc\n')
    lon, lat, val, vh, any_vh = loss.read_exposure_csv(str(fn), 70.0)
    assert lon.tolist() == [-80.19, 279.5, -75.0] and lat.tolist() == [25.76, 26.0, 35.2] and val.tolist() == [1.5e6, 2e6, 0.0]
    assert vh.tolist() == [70.0, 60.5, 70.0] and any_vh
    fn.write_text('1,2,3\n4,5,6\n')
    *_, vh, any_vh = loss.read_exposure_csv(str(fn))
    assert vh.tolist() == [74.7, 74.7] and not any_vh
    fn.write_text('nothing here\n')
    assert loss.read_exposure_csv(str(fn))[0].size == 0


# ------------------------------------------------------------------------------------------------------------------ GPU
def _sites(rng, lon, lat, n, r_out):
    """n sites uniformly random within 0.9 r_out of random track samples (none is placed at r_out), both longitude conventions."""
    live = np.argwhere(np.isfinite(lon) & np.isfinite(lat))
    pick = live[rng.choice(len(live), n, replace=False)]
    slon, slat = WN.direct(lon[pick[:, 0], pick[:, 1]], lat[pick[:, 0], pick[:, 1]], rng.uniform(2.0, 0.9 * r_out, n),
                           rng.uniform(0, 2 * np.pi, n))
    return np.where(rng.random(n) < 0.3, slon + 360.0, slon), slat


def _values(rng, n):
    value = rng.lognormal(13.0, 1.5, n)
    value[rng.random(n) < 0.15] = 0.0                                       # sites with nothing exposed
    return value


def _tile_and_chunk(slon, slat, groups, n_groups):
    """The scan's tile of every site (runs of 64 in Morton order) and chunk of every storm (runs of 16 inside a group, which is
    the chunk length below 8192 / n_tile * 16 storms)."""
    from tropical_cyclone_risk_amd import sitescan
    tile = np.empty(slon.size, np.int64)
    tile[sitescan.spatial_order(slon, slat, np)] = np.arange(slon.size) // 64
    chunk = np.empty(groups.size, np.int64)
    base = 0
    for g in range(n_groups):
        idx = np.nonzero(groups == g)[0]
        chunk[idx] = base + np.arange(idx.size) // 16
        base += (idx.size + 15) // 16
    return tile, chunk


def _check_against_site_max(r, S, value, vt, vh, groups, n_groups):
    """The fused sums against NumPy sums of T = value D(S), within the reordering bound of a sum of non-negative terms plus the
    few roundings of D; year_agg / year_max against the returned event_loss."""
    n_site, n_trk = S.shape
    T = LN.loss_matrix(S, value, vt, vh)
    ev, sl = LN.exact_sums(T, 0), LN.exact_sums(T, 1)
    err_e, err_s = np.abs(r['event_loss'] - ev), np.abs(r['site_loss'] - sl)
    print('event_loss: max err / bound = %.3g, site_loss: %.3g' % (
        (err_e / np.maximum((n_site + 16) * U * ev, 1e-300)).max(initial=0),
        (err_s / np.maximum((n_trk + 16) * U * sl, 1e-300)).max(initial=0)))
    assert r['event_loss'].shape == (n_trk,) and r['site_loss'].shape == (n_site,)
    assert (err_e <= (n_site + 16) * U * ev).all()
    assert (err_s <= (n_trk + 16) * U * sl).all()
    agg, mx, n = LN.year_table(r['event_loss'], groups, n_groups)
    assert (np.abs(r['year_agg'] - agg) <= np.maximum(n - 1, 0) * U * agg).all()
    assert np.array_equal(r['year_max'].view(np.int64), mx.view(np.int64))
    return T


@pytest.mark.gpu
def test_gpu_consistent_with_the_footprint(built_lib):
    from tropical_cyclone_risk_amd import loss, windfield
    rng = np.random.default_rng(31)
    lon, lat, v, env = TW._stress_tracks(rng)
    n_trk, n_t = lon.shape
    groups, n_groups = TW._groups(rng, n_trk)
    rm_plane = rng.uniform(8.0, 90.0, (n_trk, n_t))
    # (n_site, substeps, c, rm, r_out, per-site v_half)
    cases = [(150, 1, 1.0, None, 500.0, False), (150, 3, 0.5, 35.0, 500.0, True), (150, 6, 1.5, rm_plane, 300.0, False),
             (1, 3, 1.0, rm_plane, 400.0, False), (64, 1, 0.5, None, 500.0, True), (65, 6, 1.0, 25.0, 500.0, False)]
    for n_site, sub, c, rm, r_out, per_site in cases:
        slon, slat = _sites(rng, lon, lat, n_site, r_out)
        value = _values(rng, n_site)
        if n_site == 1:                                                     # 20 km north of the strongest sample
            k = np.unravel_index(np.nanargmax(np.where(np.isfinite(lon + lat), v, np.nan)), v.shape)
            slon, slat = WN.direct(lon[k], lat[k], 20.0, 0.0)
            slon, slat = np.array([float(slon)]), np.array([float(slat)])
            value[:] = 3.5e5
        vt = 25.7 if sub != 3 else 18.0
        vh = rng.uniform(vt + 5.0, 110.0, n_site) if per_site else 74.7
        thr = np.sort(rng.uniform(0, 90, 12))
        kw = dict(rmax_km=rm, ck_cd=c, r_out_km=r_out, substeps=sub, thresholds=thr, n_groups=n_groups)
        w = windfield.site_wind(lon, lat, v, env, groups, slon, slat, DT, return_max=True, **kw)
        r = loss.portfolio_loss(lon, lat, v, env, groups, slon, slat, value, DT, v_thresh=vt, v_half=vh, **kw)
        assert np.array_equal(r['counts'], w['counts']) and r['counts'].dtype == np.int32
        assert np.array_equal(r['thresholds'], thr) and 'site_max' not in r
        T = _check_against_site_max(r, w['site_max'], value, vt, vh, groups, n_groups)
        assert (r['event_loss'] > 0).sum() >= {1: 1, 64: 10, 65: 10, 150: 20}[n_site], (n_site, (r['event_loss'] > 0).sum())
        assert (r['event_loss'][:5] == 0).all()                             # one-sample tracks
        assert r['year_agg'][1] == 0 and r['year_agg'][4] == 0 and r['year_max'][1] == 0 and r['year_max'][4] == 0
        assert (r['site_loss'][value == 0] == 0).all()
        if n_site == 150:
            # losses come from every tile and from several chunks of storms: some site's from another tile and chunk than another's
            tile, chunk = _tile_and_chunk(slon, slat, groups, n_groups)
            i, s = np.nonzero(T > 0)
            pairs = sorted(set(zip(tile[i].tolist(), chunk[s].tolist())))
            assert len(set(tile[i])) == 3 and len(set(chunk[s])) >= 4
            assert any(a[0] != b[0] and a[1] != b[1] for a in pairs for b in pairs)
    # a threshold above every wind: every loss is exactly 0; the counts are still the footprint's
    z = loss.portfolio_loss(lon, lat, v, env, groups, slon, slat, value, DT, v_thresh=400.0, v_half=500.0, **kw)
    assert np.array_equal(z['counts'], w['counts'])
    for k in ('event_loss', 'year_agg', 'year_max', 'site_loss'):
        assert (z[k] == 0).all() and not np.signbit(z[k]).any(), k
    # no storms at all
    e = loss.portfolio_loss(lon[:0], lat[:0], v[:0], [x[:0] for x in env], groups[:0], slon, slat, value, DT, n_groups=n_groups)
    assert e['event_loss'].shape == (0,) and e['counts'].shape == (n_site, n_groups, 15) and not e['counts'].any()
    assert np.array_equal(e['year_agg'], np.zeros(n_groups)) and np.array_equal(e['year_max'], np.zeros(n_groups))
    assert np.array_equal(e['site_loss'], np.zeros(n_site))


@pytest.mark.gpu
def test_gpu_independent_of_the_gpus_own_site_max(built_lib):
    """Against the footprint's NumPy restatement: |event_loss - ref| <= sum_i value_i (TOL_ABS + TOL_REL m) / (v_half_i - v_thresh)
    (D's slope is at most 0.84 / (v_half - v_thresh); 1 / (v_half - v_thresh) is the safe form) plus the summation bound."""
    from tropical_cyclone_risk_amd import loss
    rng = np.random.default_rng(47)
    lon, lat, v, env = TW._stress_tracks(rng)
    n_trk, n_t = lon.shape
    groups, n_groups = TW._groups(rng, n_trk)
    n_site, vt = 150, 25.7
    for sub, c, rm, r_out, per_site in ((1, 1.0, None, 500.0, False), (3, 1.5, 30.0, 350.0, True)):
        slon, slat = _sites(rng, lon, lat, n_site, r_out)
        value = _values(rng, n_site)
        vh = rng.uniform(40.0, 110.0, n_site) if per_site else np.full(n_site, 74.7)
        recs = WN.samples(lon, lat, v, env, DT, rmax_km=rm, substeps=sub)
        lo, amb_any, _ = WN.site_max(recs, slon, slat, r_out, c)
        assert amb_any.sum() == 0                                           # no (site, sample) pair in the r_out band
        r = loss.portfolio_loss(lon, lat, v, env, groups, slon, slat, value, DT, v_thresh=vt, v_half=vh if per_site else 74.7,
                                rmax_km=rm, ck_cd=c, r_out_km=r_out, substeps=sub, n_groups=n_groups)
        T = LN.loss_matrix(lo, value, vt, vh)
        m = np.where(np.isnan(lo), 0.0, lo)
        slack = (value[:, None] * np.where(np.isnan(lo), 0.0, WN.TOL_ABS + WN.TOL_REL * m) / (vh[:, None] - vt))
        ev, sl = LN.exact_sums(T, 0), LN.exact_sums(T, 1)
        err_e, err_s = np.abs(r['event_loss'] - ev), np.abs(r['site_loss'] - sl)
        bound_e = slack.sum(axis=0) + (n_site + 16) * U * ev
        bound_s = slack.sum(axis=1) + (n_trk + 16) * U * sl
        print('independent: event_loss max err / bound = %.3g, site_loss %.3g'
              % ((err_e / np.maximum(bound_e, 1e-300)).max(), (err_s / np.maximum(bound_s, 1e-300)).max()))
        assert (err_e <= bound_e).all() and (err_s <= bound_s).all()
        assert (ev > 0).sum() > 30 and (ev[:5] == 0).all()
        assert (r['event_loss'][ev == 0] == 0).all()


@pytest.mark.gpu
def test_gpu_bit_identity(built_lib):
    from tropical_cyclone_risk_amd import loss
    rng = np.random.default_rng(5)
    lon, lat, v, env = TW._stress_tracks(rng)
    n_trk = lon.shape[0]
    groups, n_groups = TW._groups(rng, n_trk)
    n_site = 150
    slon, slat = _sites(rng, lon, lat, n_site, 500.0)
    value = _values(rng, n_site)
    vh = rng.uniform(40.0, 110.0, n_site)
    kw = dict(v_half=vh, r_out_km=500.0, substeps=3, n_groups=n_groups)
    keys = ('event_loss', 'year_agg', 'year_max', 'site_loss')
    a = loss.portfolio_loss(lon, lat, v, env, groups, slon, slat, value, DT, **kw)
    b = loss.portfolio_loss(lon, lat, v, env, groups, slon, slat, value, DT, **kw)
    for k in keys:
        assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k
    assert np.array_equal(a['counts'], b['counts']) and (a['event_loss'] > 0).sum() > 30
    # storms shuffled within and across groups: event losses move with their storms, bit for bit
    pt = rng.permutation(n_trk)
    d = loss.portfolio_loss(lon[pt], lat[pt], v[pt], [e[pt] for e in env], groups[pt], slon, slat, value, DT, **kw)
    assert np.array_equal(d['event_loss'].view(np.int64), a['event_loss'][pt].view(np.int64))
    assert np.array_equal(d['year_max'].view(np.int64), a['year_max'].view(np.int64))
    assert np.array_equal(d['counts'], a['counts'])
    # the storms of groups {0, 3} and of group 2 in two calls: the same event losses as in one
    first = (groups == 0) | (groups == 3)
    for sel in (first, ~first):
        p = loss.portfolio_loss(lon[sel], lat[sel], v[sel], [e[sel] for e in env], groups[sel], slon, slat, value, DT, **kw)
        assert sel.sum() > 30 and np.array_equal(p['event_loss'].view(np.int64), a['event_loss'][sel].view(np.int64))
        g_in = np.unique(groups[sel])
        assert np.array_equal(p['year_max'][g_in].view(np.int64), a['year_max'][g_in].view(np.int64))
    # sites shuffled: tiles are formed after the Morton sort and key ties may reorder, so sums may be reordered, no more
    ps = rng.permutation(n_site)
    c = loss.portfolio_loss(lon, lat, v, env, groups, slon[ps], slat[ps], value[ps], DT, **dict(kw, v_half=vh[ps]))
    assert np.array_equal(c['counts'], a['counts'][ps])
    assert (np.abs(c['event_loss'] - a['event_loss']) <= (n_site + 16) * U * a['event_loss']).all()
    assert (np.abs(c['site_loss'] - a['site_loss'][ps]) <= (n_trk + 16) * U * a['site_loss'][ps]).all()
    assert (np.abs(c['year_max'] - a['year_max']) <= (n_site + 16) * U * a['year_max']).all()
    n_in = np.bincount(groups, minlength=n_groups)
    assert (np.abs(c['year_agg'] - a['year_agg']) <= (n_site + 16 + n_in) * U * a['year_agg']).all()


@pytest.mark.gpu
def test_gpu_host_and_device_entry_points_agree(built_lib):
    import torch
    from tropical_cyclone_risk_amd import loss
    from tropical_cyclone_risk_amd.engine import TCEngine
    rng = np.random.default_rng(8)
    lon, lat, v, env = TW._stress_tracks(rng)
    n_trk, n_t = lon.shape
    groups, n_groups = TW._groups(rng, n_trk)
    slon, slat = _sites(rng, lon, lat, 150, 400.0)
    value = _values(rng, 150)
    vh = rng.uniform(40.0, 110.0, 150)
    rm = rng.uniform(10.0, 60.0, (n_trk, n_t))
    kw = dict(rmax_km=rm, ck_cd=1.5, r_out_km=400.0, substeps=4, n_groups=n_groups, v_thresh=20.0, v_half=vh)
    ref = loss.portfolio_loss(lon, lat, v, env, groups, slon, slat, value, DT, **kw)
    assert (ref['event_loss'] > 0).sum() > 30
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(x, device=dev) for x in [lon, lat, v] + env + [slon, slat, rm, value, vh]]
    eng = TCEngine('NA', device=0)
    side = torch.cuda.Stream(dev)
    try:
        for _ in range(2):
            with torch.cuda.stream(side):
                r = loss.portfolio_loss(t[0], t[1], t[2], t[3:7], groups, t[7], t[8], t[10], DT, engine=eng,
                                        **dict(kw, rmax_km=t[9], v_half=t[11]))
            side.synchronize()
            assert np.array_equal(r['counts'].cpu().numpy(), ref['counts'])
            for k in ('event_loss', 'year_agg', 'year_max', 'site_loss'):
                assert r[k].device == dev and r[k].shape == ref[k].shape
                assert np.array_equal(r[k].cpu().numpy().view(np.int64), ref[k].view(np.int64)), k
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_abi_rejects_bad_arguments(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        n_trk, n_t = 2, 6
        planes = [np.full((n_trk, n_t), x) for x in (280.0, 20.0, 60.0, 1.0, 1.0, 0.0, 0.0)]
        planes[0] = planes[0] + 0.1 * np.arange(n_t)
        off = (ctypes.c_int64 * 2)(0, n_trk)
        s = np.array([280.2, 280.4]), np.array([20.0, 20.1])
        thr = np.array([10.0, 20.0])
        counts = np.zeros((2, 1, 2), np.int32)
        ev, agg, mx, sl = np.zeros(n_trk), np.zeros(1), np.zeros(1), np.zeros(2)
        trk = _lib.WindTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=planes[0].ctypes.data, lat=planes[1].ctypes.data,
                              v=planes[2].ctypes.data, u250=planes[3].ctypes.data, v250=planes[4].ctypes.data,
                              u850=planes[5].ctypes.data, v850=planes[6].ctypes.data, rmax_km=None, n_group=1, group_off=off)

        def call(value=(1.0, 2.0), vhalf=None, wind=None, **p):
            value = np.array(value, float)
            vhalf = None if vhalf is None else np.array(vhalf, float)
            wprm = _lib.WindParams(**dict(dict(dt_s=DT, ck_cd=1.0, r_out_km=500.0, rmax_const_km=0.0, substeps=1), **(wind or {})))
            lprm = _lib.LossParams(**dict(dict(v_thresh=25.7, v_half=74.7), **p))
            return L.tcr_loss_host(h, ctypes.byref(trk), ctypes.byref(wprm), ctypes.byref(lprm), 2, s[0].ctypes.data,
                                   s[1].ctypes.data, value.ctypes.data, None if vhalf is None else vhalf.ctypes.data, 2,
                                   thr.ctypes.data_as(_lib.DP), counts.ctypes.data, ev.ctypes.data, agg.ctypes.data,
                                   mx.ctypes.data, sl.ctypes.data)
        assert call() == 0 and counts.sum() > 0 and (ev > 0).all() and agg[0] > 0
        good = [x.copy() for x in (ev, agg, mx, sl)]
        for kw, word in ((dict(value=(1.0, -2.0)), b'site_value'), (dict(value=(np.nan, 2.0)), b'site_value'),
                         (dict(vhalf=(74.7, 25.7)), b'site_v_half'), (dict(vhalf=(np.inf, 80.0)), b'site_v_half'),
                         (dict(v_thresh=np.nan), b'v_thresh'), (dict(v_thresh=-1.0), b'v_thresh'), (dict(v_half=25.7), b'v_half'),
                         (dict(v_half=np.nan), b'v_half'), (dict(wind=dict(r_out_km=2001.0)), b'r_out_km'),
                         (dict(wind=dict(substeps=65)), b'substeps'), (dict(wind=dict(ck_cd=2.0)), b'ck_cd')):
            assert call(**kw) == -1, kw
            assert word in L.tcr_last_error(h), (kw, L.tcr_last_error(h))
        # the context still serves a good call, with the same bits
        assert call() == 0
        for x, y in zip((ev, agg, mx, sl), good):
            assert np.array_equal(x.view(np.int64), y.view(np.int64))
        assert call(vhalf=(74.7, 60.0)) == 0 and sl[1] > good[3][1] and sl[0] == good[3][0]
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_run_downscaling_tracks_then_cli(golden_env, built_lib, tmp_path):
    from tropical_cyclone_risk_amd import io as tio, loss, windfield
    from tropical_cyclone_risk_amd.climatology import sample_spacing
    fn = TW._run_downscaling(golden_env, tmp_path)
    d = tio.read_tracks(fn)
    lon, lat, v = (np.asarray(d[k], float) for k in ('lon_trks', 'lat_trks', 'v_trks'))
    env = [np.asarray(d[k], float) for k in windfield.ENV_VARS]
    dt = sample_spacing([d['time']])
    groups = np.asarray(d['tc_years']).astype(int) - 2001
    i = np.argwhere(np.isfinite(lon))[::53][:8]
    slon = np.concatenate([lon[i[:, 0], i[:, 1]] - 360.0, [-80.1918]])
    slat = np.concatenate([lat[i[:, 0], i[:, 1]] + 0.7, [25.7617]])
    value = 1e6 * (1.0 + np.arange(9.0))
    vh = np.where(np.arange(9) % 2 == 0, 74.7, 60.0)
    exp = tmp_path / 'exposure.csv'
    exp.write_text('lon,lat,value,v_half\n' + ''.join('%.12f,%.12f,%.1f,%s\n' % (a, b, c, '' if h == 74.7 else '%.1f' % h)
                                                      for a, b, c, h in zip(slon, slat, value, vh)))
    out = str(tmp_path / 'loss.npz')
    cmd = [sys.executable, '-m', 'tropical_cyclone_risk_amd.loss', fn, '--exposure', str(exp), '--out', out, '--substeps', '4',
           '--v-thresh', '15', '--return-periods', '1,1.5,3,10']
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert 'average annual loss' in p.stdout and 'AEP' in p.stdout and 'OEP' in p.stdout
    z = np.load(out)
    assert set(z.files) == {'event_loss', 'year_agg', 'year_max', 'site_loss', 'loss_cost', 'counts', 'thresholds', 'aal',
                            'return_periods', 'aep', 'oep', 'site_lon', 'site_lat', 'value', 'v_half', 'v_thresh', 'total_years',
                            'r_out_km', 'substeps', 'rmax_km', 'dt_s', 'group_file', 'group_year', 'files'}
    assert int(z['total_years']) == 3 and z['group_year'].tolist() == [2001, 2002, 2003] and z['group_file'].tolist() == [0, 0, 0]
    assert np.array_equal(z['value'], value) and np.array_equal(z['v_half'], vh)
    api = loss.portfolio_loss(lon, lat, v, env, groups, z['site_lon'], z['site_lat'], value, dt, v_thresh=15.0, v_half=vh,
                              substeps=4, n_groups=3)
    for k in ('event_loss', 'year_agg', 'year_max', 'site_loss'):
        assert np.array_equal(z[k].view(np.int64), api[k].view(np.int64)), k
    assert np.array_equal(z['counts'], api['counts']) and api['year_agg'].sum() > 0
    assert float(z['aal']) == api['year_agg'].sum() / 3 == loss.average_annual_loss(api['year_agg'], 3)
    assert np.array_equal(z['loss_cost'], api['site_loss'] / 3)
    T = [1.0, 1.5, 3.0, 10.0]
    assert np.array_equal(z['return_periods'], T)
    assert np.array_equal(z['aep'], loss.loss_curve(api['year_agg'], 3, T), equal_nan=True)
    assert np.array_equal(z['oep'], loss.loss_curve(api['year_max'], 3, T), equal_nan=True)
    assert np.isnan(z['aep'][3]) and z['aep'][2] == api['year_agg'].max() and z['oep'][0] == api['year_max'].min()
    # and the sums are the footprint's: the NumPy route through site_max
    w = windfield.site_wind(lon, lat, v, env, groups, z['site_lon'], z['site_lat'], dt, substeps=4, return_max=True, n_groups=3)
    _check_against_site_max(api, w['site_max'], value, 15.0, vh, groups, 3)
