// Site wind hazard behind the C ABI (include/tcrisk_hip.h, "site hazard" section): the analysis the reference's
// notebooks/sample_analysis.ipynb runs on a track file, for many sites at once.
//
//   max[site][storm] = nanmax of vmax over the samples with haversine(site, sample) <= R   (NaN when there are none)
//   counts[site][group][bin] = #storms of the group with max >= thr[bin]
//
// A user of the site scan (tcr_sitescan.h: tiling, culling, counts).  What is the hazard's own:
//   k_hazard_prep    one wave per storm: compacts the live samples (lon and lat not NaN) to the front of the storm's row as
//                    { sin(phi/2), cos(phi/2), sin(lam/2), cos(lam/2), cos(phi), vmax, lat, lon }; the scan's row tail then writes
//                    a bounding cap (unit-vector centre, angular radius) of the storm and of every kHzSeg-sample segment of it;
//   HazardScan       the policy of k_site_scan<HazardScan>: the value of an included pair is the sample's vmax.
//
// The distance decision.  The notebook's d = 6378 * 2 * arcsin(sqrt(a)), a = sin^2(dphi/2) + cos phi1 cos phi2 sin^2(dlam/2), is
// monotone in a, so d <= R is a <= a_R = sin^2(R / (2 * 6378)) (a_R computed once on the host).  sin(dphi/2) and sin(dlam/2) are
// formed by the difference identity from the per-point half-angle terms: no trigonometry per pair, and the form is periodic in 360
// degrees of longitude, so sites and tracks may use different conventions.  At 100 km it differs from NumPy's d by ~5e-12 km.
//
// Culling (tcr_sitescan.h) changes which pairs are evaluated, never a result: max is a max of inputs (no arithmetic) and the counts
// are integers, so results are bit-identical whatever the launch shape.

namespace {

constexpr double kHzRe = 6378.0;            // r_earth of the notebook's haversine (km)

struct HzSample {                           // one live sample (64 bytes)
    double sp, cp, sl, cl, cosp, v, lat, lon;
    static __device__ __forceinline__ HzSample uniform(const HzSample *p)
    {
        const double *d = &p->sp;
        return HzSample{hz_uniform(d), hz_uniform(d + 1), hz_uniform(d + 2), hz_uniform(d + 3), hz_uniform(d + 4), hz_uniform(d + 5), 0.0, 0.0};
    }
    __device__ void centre(HzCap *out) const
    {
        const double phi = lat * (M_PI / 180.0), lam = lon * (M_PI / 180.0);
        out->x = cos(phi) * cos(lam); out->y = cos(phi) * sin(lam); out->z = sin(phi);
    }
};

struct HazardScan {
    using Rec = HzSample;
    using Mode = ScanPeak<false>;
    static constexpr int kUnroll = 4;
    __device__ __forceinline__ double value(const ScanSite &, const HzSample &p, double) const { return p.v; }
};

struct HzPrepArgs {
    const double *lon, *lat, *vmax;
    int64_t n_trk, n_t, stride;
    ScanRows<HzSample> out;
};

__global__ __launch_bounds__(64) void k_hazard_prep(HzPrepArgs a)
{
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const double *lon = a.lon + s * a.stride, *lat = a.lat + s * a.stride, *vm = a.vmax + s * a.stride;
    HzSample *row = a.out.rec + s * a.out.n_seg_max * kHzSeg;
    int n = 0;
    for (int64_t j0 = 0; j0 < a.n_t; j0 += 64) {
        const int64_t j = j0 + lane;
        double x = NAN, y = NAN, v = NAN;
        if (j < a.n_t) { x = lon[j]; y = lat[j]; v = vm[j]; }
        const bool live = !isnan(x) && !isnan(y);
        const unsigned long long m = __ballot(live);
        if (live) {
            const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
            const double hp = y * (M_PI / 360.0), hl = x * (M_PI / 360.0);      // half angles in radians
            HzSample p;
            p.sp = sin(hp); p.cp = cos(hp); p.sl = sin(hl); p.cl = cos(hl);
            p.cosp = cos(y * (M_PI / 180.0)); p.v = v; p.lat = y; p.lon = x;
            row[pos] = p;
        }
        n += __popcll(m);
    }
    scan_finish_row(a.out, s, n);
}

int hazard_check(tcr_ctx *ctx, const tcr_hazard_tracks *t, int64_t n_site, const double *site_lon, const double *site_lat,
                 double radius_km, int32_t n_bin, const double *thr, const int32_t *counts)
{
    if (!t || !site_lon || !site_lat || !thr || !counts || !t->lon || !t->lat || !t->vmax || !t->group_off)
        return fail(ctx, "tcr_hazard: NULL argument");
    if (!(radius_km > 0.0 && radius_km <= 5000.0)) return fail(ctx, "tcr_hazard: radius_km must be in (0, 5000]");
    return scan_check(ctx, "tcr_hazard", t, INT64_MAX, "n_t >= 1", n_site, n_bin, thr);
}

// For a _host entry point on tcr_hazard_tracks: *d = *t with the three planes on the device (B owns them).  No storms: nothing is
// read.  false: allocation or upload failed.
bool hazard_tracks_upload(DevBuf &B, const tcr_hazard_tracks *t, tcr_hazard_tracks *d)
{
    auto up = [&](const double *p) { return t->n_trk > 0 ? B.put(p, (size_t)t->n_trk * t->row_stride) : B.get<double>(1); };
    *d = *t;
    d->lon = up(t->lon); d->lat = up(t->lat); d->vmax = up(t->vmax);
    return d->lon && d->lat && d->vmax;
}

}  // namespace

extern "C" {

int tcr_hazard_dev(tcr_ctx *ctx, const tcr_hazard_tracks *t, int64_t n_site, const double *site_lon, const double *site_lat,
                   double radius_km, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || hazard_check(ctx, t, n_site, site_lon, site_lat, radius_km, n_bin, thresholds, counts)) return -1;
    return scan_run<HzSample>(ctx, ctx->an.hz, "tcr_hazard", t, scan_plan(t, n_site, kScanAnyChunk),
                              HazardScan::Mode::shape(n_bin, thresholds), t->n_t, 0, n_site, site_lon, site_lat, radius_km, kHzRe, counts,
                              site_max, st, [&](const ScanRows<HzSample> &rows, const ScanLaunch &L, void *) {
        HzPrepArgs p{t->lon, t->lat, t->vmax, t->n_trk, t->n_t, t->row_stride, rows};
        return scan_launch(k_hazard_prep, p, rows, L, HazardScan{});
    });
}

int tcr_hazard_host(tcr_ctx *ctx, const tcr_hazard_tracks *t, int64_t n_site, const double *site_lon, const double *site_lat,
                    double radius_km, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max)
{
    if (!enter(ctx) || hazard_check(ctx, t, n_site, site_lon, site_lat, radius_km, n_bin, thresholds, counts)) return -1;
    DevBuf B;
    tcr_hazard_tracks d;
    const ScanHostIO io = scan_host_io(B, t, n_site, site_lon, site_lat, n_bin, site_max != nullptr);
    if (!hazard_tracks_upload(B, t, &d) || !io.ok) return fail(ctx, "tcr_hazard_host: device allocation / upload failed");
    if (tcr_hazard_dev(ctx, &d, n_site, io.site_lon, io.site_lat, radius_km, n_bin, thresholds, io.counts, io.site_max, ctx->stream)) return -1;
    return scan_download(ctx, io, counts, site_max);
}

int tcr_hazard_pairs(tcr_ctx *ctx, int64_t *pairs) { return ctx ? scan_pairs(ctx, ctx->an.hz, "tcr_hazard", pairs) : -1; }

}  // extern "C"
