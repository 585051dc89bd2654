// Rainfall footprint behind the C ABI (include/tcrisk_hip.h, "rainfall footprint" section): the rain every storm leaves at every
// site, from the R-CLIPER radial rain-rate profile (Tuleya, DeMaria & Kuligowski 2007) around the centre, a function of the
// distance and of vmax alone.
//
//   TCR_RAIN_TOTAL      site_value[site][storm] = sum over the records q with haversine(site, q) <= r_out of w_q rate_q(r)   (mm)
//   TCR_RAIN_PEAK_RATE  site_value[site][storm] = max over the same records of rate_q(r)                                   (mm/h)
//   counts[site][group][bin] = #storms of the group with site_value >= thr[bin]
//
// A user of the site scan (tcr_sitescan.h: tiling, culling, counts).  What is the rainfall's own:
//   k_rain_prep      one wave per storm: finds the track (ballot), then writes one record per sample and sub-sample with every
//                    wave-uniform term a pair needs: the position's half- and full-angle terms, the profile of the record's vmax
//                    already in mm/h (T0, the inner slope (Tm - T0) / rm, Tm, rm, 1 / re) and the trapezoid weight w (hours).
//                    The three planes are read where they lie: a record needs two neighbouring samples of them and nothing
//                    derived per sample, so there is no stage buffer;
//   RainScan<SUM>    the policy of k_site_scan, with ScanPeak<SUM> for its mode.  SUM: the scan adds w rate in record order;
//                    otherwise the scan's max of rate.
//
// Per included pair:  r = 2 R asin(sqrt(a)),  rate = max(0, r < rm ? T0 + slope r : Tm exp(-(r - rm) / re)): one asin, one sqrt and
// either a multiply-add or one exp.
//
// Bit-identity: tcr_sitescan.h's argument for a sum in record order.  The sum of a (site, storm) is one lane's, over the records with a <= a_out in
// record order, whatever is culled around them; nothing here or there reduces site_value across lanes or chunks.

namespace {

constexpr int kRfMaxSub = 64;

// one sample or sub-sample (128 bytes): half-angle terms of the centre (distance), full-angle terms (the cap's centre), the
// profile in mm/h and km, and the weight in hours; then q and end, the record's index in its track and whether it is the track's
// last, which k_rain_prep fills and only the accumulation windows read (tcr_accumulation.hip)
struct RfRec {
    double sp, cp, sl, cl, cosp, t0, slope, tm, rm, ire, w, sinp, sinl, cosl;
    int64_t q, end;
    static __device__ __forceinline__ RfRec uniform(const RfRec *p)
    {
        const double *d = &p->sp;
        return RfRec{hz_uniform(d), hz_uniform(d + 1), hz_uniform(d + 2), hz_uniform(d + 3), hz_uniform(d + 4), hz_uniform(d + 5),
                     hz_uniform(d + 6), hz_uniform(d + 7), hz_uniform(d + 8), hz_uniform(d + 9), hz_uniform(d + 10), 0.0, 0.0, 0.0,
                     hz_uniform(&p->q), hz_uniform(&p->end)};
    }
    __device__ void centre(HzCap *out) const { out->x = cosp * cosl; out->y = cosp * sinl; out->z = sinp; }
};

struct RfPrepArgs {
    const double *lon, *lat, *vmax;
    int64_t n_trk, n_t, stride;
    double w;                               // dt_s / (3600 substeps): hours per sub-step
    double v_lo, v_hi, a[4], b[4];
    int32_t sub;
    ScanRows<RfRec> out;
};

__device__ __forceinline__ RfRec rf_record(const RfPrepArgs &a, double x, double y, double v, double w)
{
    RfRec r;
    const double hp = y * (kPi / 360.0), hl = x * (kPi / 360.0), phi = y * (kPi / 180.0), lam = x * (kPi / 180.0);
    r.sp = sin(hp); r.cp = cos(hp); r.sl = sin(hl); r.cl = cos(hl);
    r.cosp = cos(phi); r.sinp = sin(phi); r.sinl = sin(lam); r.cosl = cos(lam);
    const double kt = fmin(fmax(v * (3600.0 / 1852.0), a.v_lo), a.v_hi);
    const double u = 1.0 + (kt - 35.0) / 33.0;
    const double mmh = 25.4 / 24.0;                     // inches / day -> mm / h
    r.t0 = (a.a[0] + a.b[0] * u) * mmh;
    r.tm = (a.a[1] + a.b[1] * u) * mmh;
    r.rm = a.a[2] + a.b[2] * u;
    r.slope = (r.tm - r.t0) / r.rm;
    r.ire = 1.0 / (a.a[3] + a.b[3] * u);
    r.w = w;
    r.q = r.end = 0;
    return r;
}

// record q of the nr records of a track (planes at the storm's row): sample q / sub, or the sub-sample at tau = (q % sub) / sub
// after it, with the trapezoid weight of its place in the track
__device__ __forceinline__ RfRec rf_sub_record(const RfPrepArgs &a, const double *lon, const double *lat, const double *vv, int q, int nr)
{
    const int k = q / a.sub, j = q - k * a.sub;
    const double w = (q == 0 || q == nr - 1) ? 0.5 * a.w : a.w;
    const double x = lon[k], y = lat[k], v = vv[k];
    RfRec r;
    if (j == 0) r = rf_record(a, x, y, v, w);
    else {
        const double tau = (double)j / (double)a.sub;
        double dl = lon[k + 1] - x;
        dl -= 360.0 * floor((dl + 180.0) / 360.0);      // [-180, 180)
        r = rf_record(a, x + tau * dl, y + tau * (lat[k + 1] - y), v + tau * (vv[k + 1] - v), w);
    }
    r.q = q;
    r.end = q == nr - 1 ? 1 : 0;
    return r;
}

__global__ __launch_bounds__(64) void k_rain_prep(RfPrepArgs a)
{
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t o = s * a.stride;
    const double *lon = a.lon + o, *lat = a.lat + o, *vv = a.vmax + o;
    // the track: the samples before the first one with a non-finite input
    const int64_t n = scan_track_len(a.n_t, [&](int64_t j) { return !(isfinite(lon[j]) && isfinite(lat[j]) && isfinite(vv[j])); });
    RfRec *row = a.out.rec + s * a.out.n_seg_max * kHzSeg;
    const int nr = n >= 2 ? (int)((n - 1) * a.sub + 1) : 0;
    for (int q = lane; q < nr; q += 64) row[q] = rf_sub_record(a, lon, lat, vv, q, nr);
    scan_finish_row(a.out, s, nr);
}

// the policy of k_site_scan<RainScan<SUM>>: the rain rate (SUM: times the record's hours) a record produces at a site
// a = sin^2(angle / 2) away
template <bool SUM>
struct RainScan {
    using Rec = RfRec;
    using Mode = ScanPeak<SUM>;
    static constexpr int kUnroll = 2;
    __device__ __forceinline__ double value(const ScanSite &s, const RfRec &p, double q) const { return at_angle(s, p, scan_pair_angle(q)); }
    // the same from the pair's angle (radians), which a joint scan (tcr_compound.hip) forms once for two hazards
    __device__ __forceinline__ double at_angle(const ScanSite &, const RfRec &p, double ang) const
    {
        const double r = ang * (kWfEarthR / 1000.0);
        const double rate = fmax(r < p.rm ? p.t0 + p.slope * r : p.tm * exp(-(r - p.rm) * p.ire), 0.0);
        return SUM ? p.w * rate : rate;
    }
};

// the prep kernel's arguments of a call; rows: where the records go
inline RfPrepArgs rain_prep_args(const tcr_hazard_tracks *t, const tcr_rain_params *prm, const ScanRows<RfRec> &rows)
{
    return RfPrepArgs{t->lon, t->lat, t->vmax, t->n_trk, t->n_t, t->row_stride, prm->dt_s / (3600.0 * prm->substeps), prm->v_lo_kt,
                      prm->v_hi_kt, {prm->a[0], prm->a[1], prm->a[2], prm->a[3]}, {prm->b[0], prm->b[1], prm->b[2], prm->b[3]},
                      prm->substeps, rows};
}

// U of a clamp end (knots)
inline double rf_u(double kt) { return 1.0 + (kt - 35.0) / 33.0; }

// who: the prefix of the messages (tcr_compound.hip runs the same rules under its own name)
int rainfall_check(tcr_ctx *ctx, const tcr_hazard_tracks *t, const tcr_rain_params *p, int64_t n_site, const double *site_lon,
                   const double *site_lat, int32_t n_bin, const double *thr, const int32_t *counts, const char *who = "tcr_rainfall")
{
    if (!t || !p || !site_lon || !site_lat || !thr || !counts || !t->lon || !t->lat || !t->vmax || !t->group_off)
        return fail(ctx, "%s: NULL argument", who);
    if (!(p->dt_s > 0.0 && std::isfinite(p->dt_s))) return fail(ctx, "%s: dt_s must be finite and > 0", who);
    if (!(p->r_out_km > 0.0 && p->r_out_km <= 2000.0)) return fail(ctx, "%s: r_out_km must be in (0, 2000]", who);
    if (p->substeps < 1 || p->substeps > kRfMaxSub) return fail(ctx, "%s: substeps must be in [1, 64]", who);
    if (p->stat != TCR_RAIN_TOTAL && p->stat != TCR_RAIN_PEAK_RATE)
        return fail(ctx, "%s: stat must be TCR_RAIN_TOTAL (0) or TCR_RAIN_PEAK_RATE (1)", who);
    if (!(p->v_lo_kt > 0.0 && p->v_lo_kt <= p->v_hi_kt && std::isfinite(p->v_hi_kt)))
        return fail(ctx, "%s: need 0 < v_lo_kt <= v_hi_kt, both finite", who);
    for (int i = 0; i < 4; ++i)
        if (!(std::isfinite(p->a[i]) && std::isfinite(p->b[i]))) return fail(ctx, "%s: the coefficients must be finite", who);
    // Tm, rm and re are linear in U: what holds at both clamp ends holds in between
    for (const double kt : {p->v_lo_kt, p->v_hi_kt}) {
        const double u = rf_u(kt);
        if (!(p->a[2] + p->b[2] * u > 0.0 && p->a[3] + p->b[3] * u > 0.0 && p->a[1] + p->b[1] * u >= 0.0))
            return fail(ctx, "%s: the coefficients must give rm > 0, re > 0 and Tm >= 0 at v_lo_kt and at v_hi_kt", who);
    }
    return scan_check(ctx, who, t, 1 << 20, "1 <= n_t <= 2^20", n_site, n_bin, thr);
}

}  // namespace

extern "C" {

int tcr_rainfall_dev(tcr_ctx *ctx, const tcr_hazard_tracks *t, const tcr_rain_params *prm, int64_t n_site, const double *site_lon,
                     const double *site_lat, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_value, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || rainfall_check(ctx, t, prm, n_site, site_lon, site_lat, n_bin, thresholds, counts)) return -1;
    const int64_t n_rec = (t->n_t - 1) * prm->substeps + 1;
    // (both stats' modes have the one shape)
    return scan_run<RfRec>(ctx, ctx->an.rf, "tcr_rainfall", t, scan_plan(t, n_site, kScanAnyChunk), ScanPeak<true>::shape(n_bin, thresholds),
                           n_rec, 0, n_site, site_lon, site_lat, prm->r_out_km, kWfEarthR / 1000.0, counts, site_value, st,
                           [&](const ScanRows<RfRec> &rows, const ScanLaunch &L, void *) {
        const RfPrepArgs p = rain_prep_args(t, prm, rows);
        if (prm->stat == TCR_RAIN_TOTAL) return scan_launch(k_rain_prep, p, rows, L, RainScan<true>{});
        return scan_launch(k_rain_prep, p, rows, L, RainScan<false>{});
    });
}

int tcr_rainfall_host(tcr_ctx *ctx, const tcr_hazard_tracks *t, const tcr_rain_params *prm, int64_t n_site, const double *site_lon,
                      const double *site_lat, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_value)
{
    if (!enter(ctx) || rainfall_check(ctx, t, prm, n_site, site_lon, site_lat, n_bin, thresholds, counts)) return -1;
    DevBuf B;
    tcr_hazard_tracks d;
    const ScanHostIO io = scan_host_io(B, t, n_site, site_lon, site_lat, n_bin, site_value != nullptr);
    if (!hazard_tracks_upload(B, t, &d) || !io.ok) return fail(ctx, "tcr_rainfall_host: device allocation / upload failed");
    if (tcr_rainfall_dev(ctx, &d, prm, n_site, io.site_lon, io.site_lat, n_bin, thresholds, io.counts, io.site_max, ctx->stream)) return -1;
    return scan_download(ctx, io, counts, site_value);
}

int tcr_rainfall_pairs(tcr_ctx *ctx, int64_t *pairs) { return ctx ? scan_pairs(ctx, ctx->an.rf, "tcr_rainfall", pairs) : -1; }

}  // extern "C"
