// Wind footprint behind the C ABI (include/tcrisk_hip.h, "wind footprint" section): the peak wind every storm produces at every
// site, from the Emanuel & Rotunno (2011, eq. 36) radial profile around the centre plus the asymmetry of axi_to_max_wind
// (wind/tc_wind.py), so that at r = rm on the azimuth of maximum wind it is the pipeline's vmax_trks.
//
//   site_max[site][storm] = max over the samples and sub-samples with haversine(site, centre) <= r_out of |V(r) t + (V / v) A|
//   counts[site][group][bin] = #storms of the group with site_max >= thr[bin]
//
// A user of the site scan (tcr_sitescan.h: tiling, culling, counts).  What is the footprint's own:
//   k_wind_prep      one wave per storm: finds the track (ballot), stages (lon, lat, v, rm, A) of every track sample with the
//                    translation speed in the operation order of vmax_at (tcr_kernels.hip), then writes one record per sample and
//                    sub-sample with every wave-uniform term a pair needs (and its trapezoid half-weight); the scan's row tail writes the bounding caps of the
//                    storm and of every kHzSeg-record segment;
//   WindScan<c == 1> the policy of k_site_scan: the scan tests the haversine argument a against a_out first (no trigonometry), so
//                    only included lanes pay for asin, the square roots and the profile.  from_angle is at_angle with the direction
//                    the wind blows from (tcr_directional.hip).
//
// Per included pair (c: centre, s: site; the record holds the centre's terms):
//   r = 2 R asin(sqrt(a))
//   V = r (2 Mm / (rm^2 + r^2) - f/2)            c = 1: ratio = 2 x^2 / (1 + x^2), no pow (the launch-uniform template branch)
//   V = (Mm ratio - (f/2) r^2) / r, V(0) = 0     otherwise
//   |w| = V |t + A / v| = V sqrt(1 + |A / v|^2 + d_e b_n - d_n b_e),  b = 2 h A / v
// with sin and cos of (lam_s - lam_c) from the difference identity of the full-angle terms.  |A| = min(|U|, v / 2), so the root's
// argument is >= 1/4.  A sample with v <= 0 carries Mm = f/2 = 0 and b = 0: its wind is 0 wherever it is included.
//
// Culling is the scan's (caps padded by kHzPad, test margin kHzDotPad), so a skipped pair is always farther than r_out.  A pair's
// value does not depend on which other pairs are evaluated, and max and integer sums do not depend on order: the results are
// bit-identical whatever the launch shape, the site order and the storm order.

namespace {

constexpr int kWfMaxSub = 64;
constexpr double kWfEarthR = 6.3781 * 1e6;          // util/constants.py earth_R (m): the pipeline's P.earth_R
constexpr double kWfOmega = 7.292e-5;               // s^-1

struct WfStage { double lon, lat, v, rm, ae, an, pad0, pad1; };      // one track sample (64 bytes)
// one sample or sub-sample (128 bytes): half-angle terms of the centre (distance), full-angle terms (direction), rm (m), Mm, f / 2,
// 1 + |A / v|^2 and b = 2 h A / v; then hw, the record's trapezoid half-weight (2, or 1 for a track's first and last record),
// which k_wind_prep fills and only tcr_duration.hip reads
struct WfRec {
    double sp, cp, sl, cl, cosp, sinp, sinl, cosl, rm, mm, f2, a2, be, bn;
    int64_t hw;
    double pad1;
    static __device__ __forceinline__ WfRec uniform(const WfRec *p)
    {
        const double *d = &p->sp;
        return WfRec{hz_uniform(d), hz_uniform(d + 1), hz_uniform(d + 2), hz_uniform(d + 3), hz_uniform(d + 4), hz_uniform(d + 5),
                     hz_uniform(d + 6), hz_uniform(d + 7), hz_uniform(d + 8), hz_uniform(d + 9), hz_uniform(d + 10), hz_uniform(d + 11),
                     hz_uniform(d + 12), hz_uniform(d + 13), hz_uniform(&p->hw), 0.0};
    }
    __device__ void centre(HzCap *out) const { out->x = cosp * cosl; out->y = cosp * sinl; out->z = sinp; }
};

struct WfPrepArgs {
    const double *lon, *lat, *v, *u250, *v250, *u850, *v850, *rmax;   // rmax: [n_trk][stride] km, or NULL
    int64_t n_trk, n_t, stride;
    double dt, rm_const;                    // rm_const > 0: rm everywhere (km); 0: Willoughby et al. (2006)
    int32_t sub;
    WfStage *stage;                         // [n_trk][n_t]
    ScanRows<WfRec> out;
};

// haversine_same_lat_km / haversine_same_lon_km / vmax_at of tcr_kernels.hip with R = kWfEarthR and dt = dt_s, same operations in
// the same order (the build has no contraction), up to the asymmetry vector A = fac (Ui, Vi)
__device__ __forceinline__ double wf_hav_same_lat_km(double lon1, double lon2, double lat)
{
    const double d = kPi / 180.0;
    lon1 *= d; lon2 *= d; lat *= d;
    const double sb = sin((lon2 - lon1) / 2.0), c = cos(lat);
    const double aa = 0.0 + c * c * (sb * sb);
    return (kWfEarthR / 1000.) * (2.0 * asin(sqrt(aa)));
}

__device__ __forceinline__ double wf_hav_same_lon_km(double lat1, double lat2)
{
    const double d = kPi / 180.0;
    lat1 *= d; lat2 *= d;
    const double sa = sin((lat2 - lat1) / 2.0);
    const double aa = sa * sa;
    return (kWfEarthR / 1000.) * (2.0 * asin(sqrt(aa)));
}

__device__ __forceinline__ void wf_asym(double dt, double lat, double v, double us, double vs, double lom, double lam, double lop,
                                        double lap, double &ae, double &an)
{
    const double dlon = 0.5 * (sign_of(lop - lom) * wf_hav_same_lat_km(lop, lom, lat));
    const double dlat = 0.5 * (sign_of(lap - lam) * wf_hav_same_lon_km(lap, lam));
    const double ut = dlon * 1000. / dt, vt = dlat * 1000. / dt;
    const double G = fmin(1., 0.8 + 0.35 * (1. + tanh((lat - 35.) / 10.)));
    const double Ui = G * ut + 0.1 * us * v / 15.;
    const double Vi = G * vt + 0.1 * vs * v / 15.;
    const double mag = sqrt(Ui * Ui + Vi * Vi);
    const double fac = np_min((v * 0.50) / mag, 1.0);
    ae = fac * Ui; an = fac * Vi;
}

__device__ __forceinline__ WfRec wf_record(double x, double y, double v, double rm_km, double ae, double an)
{
    WfRec r;
    const double hp = y * (kPi / 360.0), hl = x * (kPi / 360.0), phi = y * (kPi / 180.0), lam = x * (kPi / 180.0);
    r.sp = sin(hp); r.cp = cos(hp); r.sl = sin(hl); r.cl = cos(hl);
    r.cosp = cos(phi); r.sinp = sin(phi); r.sinl = sin(lam); r.cosl = cos(lam);
    r.rm = rm_km * 1000.0;
    r.hw = 0; r.pad1 = 0.0;
    if (v > 0.0) {
        const double f2 = kWfOmega * fabs(r.sinp);          // f / 2
        const double h2 = y >= 0.0 ? 2.0 : -2.0;            // 2 h
        const double ax = ae / v, ay = an / v;
        r.mm = r.rm * v + f2 * (r.rm * r.rm);
        r.f2 = f2;
        r.a2 = 1.0 + (ax * ax + ay * ay);
        r.be = h2 * ax; r.bn = h2 * ay;
    } else {
        r.mm = 0.0; r.f2 = 0.0; r.a2 = 1.0; r.be = 0.0; r.bn = 0.0;
    }
    return r;
}

// the stage entry of sample k of a track of n >= 2 samples that begins at offset o of the planes: position, intensity, rm and A, with
// the neighbour and end-extrapolation rules of k_emit; bad_rm is set when rm is not finite and > 0
__device__ __forceinline__ WfStage wf_stage(const WfPrepArgs &a, int64_t o, int64_t k, int64_t n, bool &bad_rm)
{
    const double *lon = a.lon + o, *lat = a.lat + o;
    const double x = lon[k], y = lat[k], v = a.v[o + k];
    double lom = 0.0, lam = 0.0, lop = 0.0, lap = 0.0;
    if (k > 0) { lom = lon[k - 1]; lam = lat[k - 1]; }
    if (k < n - 1) { lop = lon[k + 1]; lap = lat[k + 1]; }
    const double lop_in = lop, lap_in = lap, lom_in = lom, lam_in = lam;
    if (k == 0) { lom = 2.0 * x - lop_in; lam = 2.0 * y - lap_in; }
    if (k == n - 1) { lop = 2.0 * x - lom_in; lap = 2.0 * y - lam_in; }
    double ae, an;
    wf_asym(a.dt, y, v, a.u250[o + k] - a.u850[o + k], a.v250[o + k] - a.v850[o + k], lom, lam, lop, lap, ae, an);
    const double rm = a.rmax ? a.rmax[o + k] : (a.rm_const > 0.0 ? a.rm_const : 46.4 * exp(-0.0155 * v + 0.0169 * fabs(y)));
    if (!(isfinite(rm) && rm > 0.0)) bad_rm = true;
    return WfStage{x, y, v, rm, ae, an, 0.0, 0.0};
}

// record q of a staged track: sample q / sub, or the sub-sample at tau = (q % sub) / sub after it
__device__ __forceinline__ WfRec wf_sub_record(const WfStage *st, int q, int sub)
{
    const int k = q / sub, j = q - k * sub;
    const WfStage p = st[k];
    if (j == 0) return wf_record(p.lon, p.lat, p.v, p.rm, p.ae, p.an);
    const WfStage p1 = st[k + 1];
    const double tau = (double)j / (double)sub;
    double dl = p1.lon - p.lon;
    dl -= 360.0 * floor((dl + 180.0) / 360.0);          // [-180, 180)
    return wf_record(p.lon + tau * dl, p.lat + tau * (p1.lat - p.lat), p.v + tau * (p1.v - p.v), p.rm + tau * (p1.rm - p.rm),
                     p.ae + tau * (p1.ae - p.ae), p.an + tau * (p1.an - p.an));
}

__global__ __launch_bounds__(64) void k_wind_prep(WfPrepArgs a)
{
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t o = s * a.stride;
    // the track: the samples before the first one with a non-finite input
    const int64_t n = scan_track_len(a.n_t, [&](int64_t j) {
        return !(isfinite(a.lon[o + j]) && isfinite(a.lat[o + j]) && isfinite(a.v[o + j]) && isfinite(a.u250[o + j]) &&
                 isfinite(a.v250[o + j]) && isfinite(a.u850[o + j]) && isfinite(a.v850[o + j]));
    });
    WfStage *st = a.stage + s * a.n_t;
    WfRec *row = a.out.rec + s * a.out.n_seg_max * kHzSeg;
    bool bad_rm = false;
    if (n >= 2)
        for (int64_t k = lane; k < n; k += 64) st[k] = wf_stage(a, o, k, n, bad_rm);
    const bool drop = __ballot(bad_rm) != 0;
    const int nr = (n >= 2 && !drop) ? (int)((n - 1) * a.sub + 1) : 0;
    __syncthreads();                                    // the records read stage entries other lanes wrote
    for (int q = lane; q < nr; q += 64) {
        WfRec r = wf_sub_record(st, q, a.sub);
        r.hw = q == 0 || q == nr - 1 ? 1 : 2;
        row[q] = r;
    }
    scan_finish_row(a.out, s, nr);
}

// the policy of k_site_scan<WindScan<UNIT_C>>: the wind a record produces at a site a = sin^2(angle / 2) away (header comment)
template <bool UNIT_C>
struct WindScan {
    using Rec = WfRec;
    using Mode = ScanPeak<false>;
    static constexpr int kUnroll = 2;
    double c, two_c, inv_exp;               // profile: c, 2 - c, 1 / (2 - c)
    __device__ __forceinline__ double value(const ScanSite &s, const WfRec &p, double q) const { return at_angle(s, p, scan_pair_angle(q)); }
    // the same from the pair's angle (radians), which a joint scan (tcr_compound.hip) forms once for two hazards
    __device__ __forceinline__ double at_angle(const ScanSite &s, const WfRec &p, double ang) const
    {
        const double r = ang * kWfEarthR;
        double V;
        if (UNIT_C) {
            V = r * (2.0 * p.mm / (p.rm * p.rm + r * r) - p.f2);
        } else {
            const double xr = r / p.rm, x2 = xr * xr;
            V = r > 0.0 ? (p.mm * pow(2.0 * x2 / (two_c + c * x2), inv_exp) - p.f2 * (r * r)) / r : 0.0;
        }
        V = fmax(V, 0.0);
        const double sdl = s.sinl * p.cosl - s.cosl * p.sinl, cdl = s.cosl * p.cosl + s.sinl * p.sinl;
        const double e = s.cosp * sdl, nn = p.cosp * s.sinp - p.sinp * (s.cosp * cdl);
        const double dd = e * e + nn * nn;
        const double cross = dd > 0.0 ? (e * p.bn - nn * p.be) / sqrt(dd) : 0.0;
        return V * sqrt(p.a2 + cross);
    }
    // The same with the direction the wind blows from (tcr_directional.hip).  The speed is at_angle's own expressions in at_angle's
    // order (the build has no contraction), so it is at_angle's double bit for bit.  (fe, fn) = -sqrt(dd) (g_e, g_n) with
    // g = h (-d_n + be / 2, d_e + bn / 2): a positive multiple of (-w_e, -w_n) wherever the speed is > 0, east and north.  h is the
    // record's hemisphere sign from sinp: that is wf_record's `y >= 0` (-0.0 included) for every latitude whose radians are not
    // rounded to zero, which leaves the 28 negative subnormals above -28 * 2^-1074 degrees.  dd == 0 (the site on the centre, where
    // V = 0): no direction, and 0.
    __device__ __forceinline__ double from_angle(const ScanSite &s, const WfRec &p, double ang, double &fe, double &fn) const
    {
        const double r = ang * kWfEarthR;
        double V;
        if (UNIT_C) {
            V = r * (2.0 * p.mm / (p.rm * p.rm + r * r) - p.f2);
        } else {
            const double xr = r / p.rm, x2 = xr * xr;
            V = r > 0.0 ? (p.mm * pow(2.0 * x2 / (two_c + c * x2), inv_exp) - p.f2 * (r * r)) / r : 0.0;
        }
        V = fmax(V, 0.0);
        const double sdl = s.sinl * p.cosl - s.cosl * p.sinl, cdl = s.cosl * p.cosl + s.sinl * p.sinl;
        const double e = s.cosp * sdl, nn = p.cosp * s.sinp - p.sinp * (s.cosp * cdl);
        const double dd = e * e + nn * nn;
        const double sd = sqrt(dd);
        const double cross = dd > 0.0 ? (e * p.bn - nn * p.be) / sd : 0.0;
        const double h = p.sinp >= 0.0 ? 1.0 : -1.0;
        fe = h * (nn - 0.5 * p.be * sd);
        fn = -h * (e + 0.5 * p.bn * sd);
        return dd > 0.0 ? V * sqrt(p.a2 + cross) : 0.0;
    }
};

// who: the prefix of the messages (tcr_compound.hip runs the same rules under its own name)
int windfield_check(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *p, int64_t n_site, const double *site_lon,
                    const double *site_lat, int32_t n_bin, const double *thr, const int32_t *counts, const char *who = "tcr_windfield")
{
    if (!t || !p || !site_lon || !site_lat || !thr || !counts || !t->lon || !t->lat || !t->v || !t->u250 || !t->v250 || !t->u850 ||
        !t->v850 || !t->group_off)
        return fail(ctx, "%s: NULL argument", who);
    if (!(p->dt_s > 0.0 && std::isfinite(p->dt_s))) return fail(ctx, "%s: dt_s must be finite and > 0", who);
    if (!(p->ck_cd > 0.0 && p->ck_cd < 2.0)) return fail(ctx, "%s: ck_cd must be in (0, 2)", who);
    if (!(p->r_out_km > 0.0 && p->r_out_km <= 2000.0)) return fail(ctx, "%s: r_out_km must be in (0, 2000]", who);
    if (p->substeps < 1 || p->substeps > kWfMaxSub) return fail(ctx, "%s: substeps must be in [1, 64]", who);
    if (!(p->rmax_const_km >= 0.0 && std::isfinite(p->rmax_const_km)) || (t->rmax_km && p->rmax_const_km != 0.0))
        return fail(ctx, "%s: rmax_const_km must be finite and >= 0, and 0 when the rmax_km plane is given", who);
    return scan_check(ctx, who, t, 1 << 20, "1 <= n_t <= 2^20", n_site, n_bin, thr);
}

// the prep kernel's arguments of a call: stage is the [n_trk][n_t] workspace, rows where the records go
inline WfPrepArgs wind_prep_args(const tcr_wind_tracks *t, const tcr_wind_params *prm, void *stage, const ScanRows<WfRec> &rows)
{
    return WfPrepArgs{t->lon, t->lat, t->v, t->u250, t->v250, t->u850, t->v850, t->rmax_km, t->n_trk, t->n_t, t->row_stride,
                      prm->dt_s, prm->rmax_const_km, prm->substeps, static_cast<WfStage *>(stage), rows};
}

// the profile parameters of WindScan<c == 1> from ck_cd
template <bool UNIT_C>
WindScan<UNIT_C> wind_scan(const tcr_wind_params *prm) { return WindScan<UNIT_C>{prm->ck_cd, 2.0 - prm->ck_cd, 1.0 / (2.0 - prm->ck_cd)}; }

// The launch step of scan_run for every analysis on the footprint's records: the footprint's prep kernel, then Policy's scan.
template <typename Policy>
hipError_t wind_scan_launch(const tcr_wind_tracks *t, const tcr_wind_params *prm, const ScanRows<WfRec> &rows, const ScanLaunch &L,
                            void *stage, const Policy &pol)
{
    return scan_launch(k_wind_prep, wind_prep_args(t, prm, stage, rows), rows, L, pol);
}

// What a _host entry point checks and a _dev one cannot report: the rmax_km plane (when given) is finite and > 0 at every sample
// of a track (host planes)
bool wind_rmax_ok(const tcr_wind_tracks *t)
{
    if (!t->rmax_km) return true;
    const double *planes[7] = {t->lon, t->lat, t->v, t->u250, t->v250, t->u850, t->v850};
    for (int64_t s = 0; s < t->n_trk; ++s) {
        const int64_t o = s * t->row_stride;
        int64_t n = 0;
        while (n < t->n_t) {
            bool ok = true;
            for (const double *p : planes) ok = ok && std::isfinite(p[o + n]);
            if (!ok) break;
            ++n;
        }
        for (int64_t k = 0; n >= 2 && k < n; ++k)
            if (!(std::isfinite(t->rmax_km[o + k]) && t->rmax_km[o + k] > 0.0)) return false;
    }
    return true;
}

// For a _host entry point on tcr_wind_tracks: *d = *t with the seven planes (eight with rmax_km) on the device (B owns them).  No
// storms: nothing is read.  false: allocation or upload failed.
bool wind_tracks_upload(DevBuf &B, const tcr_wind_tracks *t, tcr_wind_tracks *d)
{
    auto up = [&](const double *p) { return t->n_trk > 0 ? B.put(p, (size_t)t->n_trk * t->row_stride) : B.get<double>(1); };
    *d = *t;
    d->lon = up(t->lon); d->lat = up(t->lat); d->v = up(t->v);
    d->u250 = up(t->u250); d->v250 = up(t->v250); d->u850 = up(t->u850); d->v850 = up(t->v850);
    d->rmax_km = t->rmax_km ? up(t->rmax_km) : nullptr;
    return d->lon && d->lat && d->v && d->u250 && d->v250 && d->u850 && d->v850 && (!t->rmax_km || d->rmax_km);
}

}  // namespace

extern "C" {

int tcr_windfield_dev(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                      const double *site_lat, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || windfield_check(ctx, t, prm, n_site, site_lon, site_lat, n_bin, thresholds, counts)) return -1;
    const int64_t n_rec = (t->n_t - 1) * prm->substeps + 1;
    const size_t n_stage = (size_t)std::max<int64_t>(1, t->n_trk * t->n_t);
    return scan_run<WfRec>(ctx, ctx->an.wf, "tcr_windfield", t, scan_plan(t, n_site, kScanAnyChunk),
                           ScanPeak<false>::shape(n_bin, thresholds), n_rec, n_stage * sizeof(WfStage), n_site, site_lon, site_lat,
                           prm->r_out_km, kWfEarthR / 1000.0, counts, site_max, st,
                           [&](const ScanRows<WfRec> &rows, const ScanLaunch &L, void *stage) {
        if (prm->ck_cd == 1.0) return wind_scan_launch(t, prm, rows, L, stage, wind_scan<true>(prm));
        return wind_scan_launch(t, prm, rows, L, stage, wind_scan<false>(prm));
    });
}

int tcr_windfield_host(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                       const double *site_lat, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max)
{
    if (!enter(ctx) || windfield_check(ctx, t, prm, n_site, site_lon, site_lat, n_bin, thresholds, counts)) return -1;
    if (!wind_rmax_ok(t)) return fail(ctx, "tcr_windfield_host: rmax_km must be finite and > 0 at every sample of a track");
    DevBuf B;
    tcr_wind_tracks d;
    const ScanHostIO io = scan_host_io(B, t, n_site, site_lon, site_lat, n_bin, site_max != nullptr);
    if (!wind_tracks_upload(B, t, &d) || !io.ok) return fail(ctx, "tcr_windfield_host: device allocation / upload failed");
    if (tcr_windfield_dev(ctx, &d, prm, n_site, io.site_lon, io.site_lat, n_bin, thresholds, io.counts, io.site_max, ctx->stream)) return -1;
    return scan_download(ctx, io, counts, site_max);
}

int tcr_windfield_pairs(tcr_ctx *ctx, int64_t *pairs) { return ctx ? scan_pairs(ctx, ctx->an.wf, "tcr_windfield", pairs) : -1; }

}  // extern "C"
