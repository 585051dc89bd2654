// Compound wind-rain hazard behind the C ABI (include/tcrisk_hip.h, "compound hazard" section): how many storms bring a site a
// footprint wind of at least u AND a storm rain of at least p, for every pair of thresholds, from one scan of the ensemble.
//
//   W = site_wind[site][storm]   what tcr_windfield_* writes to site_max with the call's tcr_wind_params
//   P = site_rain[site][storm]   what tcr_rainfall_* writes to site_value with the call's tcr_rain_params on (lon, lat, vmax)
//   counts[site][group][a][b]  = #storms of the group with at least a wind thresholds <= W and at least b rain thresholds <= P
//
// on the track both hazards share: the leading run of samples where all eight planes (the footprint's seven and vmax) are finite.
// The [n_site][n_trk] planes that would carry W and P to a joint count elsewhere are optional here: the histogram is built where
// the two values are still in registers.
//
// A user of the site scan (tcr_sitescan.h: tiling, culling, counts; its kJoint variant).  What is the compound's own:
//   CpRec             one sample or sub-sample (160 bytes): the position terms once, then the wind terms of WfRec and the rain
//                     terms of RfRec;
//   k_compound_prep   one wave per storm: finds the track over the eight planes (ballot), stages the footprint's per-sample terms
//                     (wf_stage), then writes one record per sample and sub-sample: wf_sub_record and rf_sub_record side by side;
//   CompoundScan      the policy of k_site_scan: WindScan's value under the wind radius, RainScan's under the rain radius, on the
//                     one angle the scan forms per included pair.
// No formula is restated here: records, interpolation and per-pair values are the footprint's and the rainfall's own functions.
//
// Bit-identity: tcr_sitescan.h's argument for kJoint.  A record's position terms are the same bits in wf_sub_record and
// rf_sub_record (the same expressions of the same lon, lat and tau; the build has no contraction), so keeping the footprint's
// copy changes nothing for the rain.  With all eight planes finite on a storm's track W and P are bit for bit the two entry
// points' outputs, whatever the launch shape, the site order and the storm order; the counts are integers.

namespace {

struct CpRec {
    double sp, cp, sl, cl, cosp, sinp, sinl, cosl;      // the centre: half-angle terms (distance), full-angle terms (direction, cap)
    double wrm, mm, f2, a2, be, bn;                     // WfRec: rm (m), Mm, f / 2, 1 + |A / v|^2, b
    double t0, slope, tm, rrm, ire, w;                  // RfRec: the profile in mm/h and km, the weight in hours
    static __device__ __forceinline__ CpRec uniform(const CpRec *p)
    {
        const double *d = &p->sp;
        return CpRec{hz_uniform(d), hz_uniform(d + 1), hz_uniform(d + 2), hz_uniform(d + 3), hz_uniform(d + 4), hz_uniform(d + 5),
                     hz_uniform(d + 6), hz_uniform(d + 7), hz_uniform(d + 8), hz_uniform(d + 9), hz_uniform(d + 10), hz_uniform(d + 11),
                     hz_uniform(d + 12), hz_uniform(d + 13), hz_uniform(d + 14), hz_uniform(d + 15), hz_uniform(d + 16),
                     hz_uniform(d + 17), hz_uniform(d + 18), hz_uniform(d + 19)};
    }
    static __device__ __forceinline__ CpRec join(const WfRec &a, const RfRec &b)
    {
        return CpRec{a.sp, a.cp, a.sl, a.cl, a.cosp, a.sinp, a.sinl, a.cosl, a.rm, a.mm, a.f2, a.a2, a.be, a.bn,
                     b.t0, b.slope, b.tm, b.rm, b.ire, b.w};
    }
    __device__ __forceinline__ WfRec wind() const { return WfRec{sp, cp, sl, cl, cosp, sinp, sinl, cosl, wrm, mm, f2, a2, be, bn, 0.0, 0.0}; }
    __device__ __forceinline__ RfRec rain() const { return RfRec{sp, cp, sl, cl, cosp, t0, slope, tm, rrm, ire, w, sinp, sinl, cosl, 0.0, 0.0}; }
    __device__ void centre(HzCap *out) const { out->x = cosp * cosl; out->y = cosp * sinl; out->z = sinp; }
};

// the two parents' prep arguments on the same rows (their `out` members are not used), and the joint rows
struct CpPrepArgs {
    WfPrepArgs wf;
    RfPrepArgs rf;
    ScanRows<CpRec> out;
};

__global__ __launch_bounds__(64) void k_compound_prep(CpPrepArgs a)
{
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t o = s * a.wf.stride;
    const double *lon = a.rf.lon + o, *lat = a.rf.lat + o, *vm = a.rf.vmax + o;
    // the track: the samples before the first one where one of the eight planes is not finite
    const int64_t n = scan_track_len(a.wf.n_t, [&](int64_t j) {
        return !(isfinite(lon[j]) && isfinite(lat[j]) && isfinite(a.wf.v[o + j]) && isfinite(a.wf.u250[o + j]) &&
                 isfinite(a.wf.v250[o + j]) && isfinite(a.wf.u850[o + j]) && isfinite(a.wf.v850[o + j]) && isfinite(vm[j]));
    });
    WfStage *st = a.wf.stage + s * a.wf.n_t;
    CpRec *row = a.out.rec + s * a.out.n_seg_max * kHzSeg;
    bool bad_rm = false;
    if (n >= 2)
        for (int64_t k = lane; k < n; k += 64) st[k] = wf_stage(a.wf, o, k, n, bad_rm);
    const bool drop = __ballot(bad_rm) != 0;            // a bad rm drops the storm, as in k_wind_prep: no records, NaN on both planes
    const int nr = (n >= 2 && !drop) ? (int)((n - 1) * a.wf.sub + 1) : 0;
    __syncthreads();                                    // the records read stage entries other lanes wrote
    for (int q = lane; q < nr; q += 64) row[q] = CpRec::join(wf_sub_record(st, q, a.wf.sub), rf_sub_record(a.rf, lon, lat, vm, q, nr));
    scan_finish_row(a.out, s, nr);
}

// the policy of k_site_scan<CompoundScan<UNIT_C, SUM>>: the kJoint variant with the footprint's wind first and the rainfall's value
// (SUM: the storm total, otherwise the peak rate) second
template <bool UNIT_C, bool SUM>
struct CompoundScan {
    using Rec = CpRec;
    static constexpr int kUnroll = 2;
    static constexpr bool kJoint = true;
    static constexpr bool kSecondSum = SUM;
    WindScan<UNIT_C> wind;
    double a_first, a_second;               // a thresholds of wind.r_out_km and rain.r_out_km
    int32_t n_first, n_second;              // n_wbin, n_rbin
    double *site_second;                    // site_rain [n_site][n_trk] or NULL
    __device__ __forceinline__ double first(const ScanSite &s, const CpRec &p, double ang) const { return wind.at_angle(s, p.wind(), ang); }
    __device__ __forceinline__ double second(const ScanSite &s, const CpRec &p, double ang) const
    {
        return RainScan<SUM>{}.at_angle(s, p.rain(), ang);
    }
};

// the rainfall's view of a compound call's tracks
inline tcr_hazard_tracks compound_rain_tracks(const tcr_wind_tracks *t, const double *vmax)
{
    return tcr_hazard_tracks{t->n_trk, t->n_t, t->row_stride, t->lon, t->lat, vmax, t->n_group, t->group_off};
}

int compound_check(tcr_ctx *ctx, const tcr_wind_tracks *t, const double *vmax, const tcr_wind_params *wp, const tcr_rain_params *rp,
                   int64_t n_site, const double *site_lon, const double *site_lat, int32_t n_wbin, const double *wthr, int32_t n_rbin,
                   const double *rthr, const int32_t *counts)
{
    if (!t || !vmax || !wp || !rp || !wthr || !rthr) return fail(ctx, "tcr_compound: NULL argument");
    if (windfield_check(ctx, t, wp, n_site, site_lon, site_lat, n_wbin, wthr, counts, "tcr_compound")) return -1;
    const tcr_hazard_tracks ht = compound_rain_tracks(t, vmax);
    if (rainfall_check(ctx, &ht, rp, n_site, site_lon, site_lat, n_rbin, rthr, counts, "tcr_compound")) return -1;
    if (wp->dt_s != rp->dt_s || wp->substeps != rp->substeps)
        return fail(ctx, "tcr_compound: the wind and the rain parameters must have the same dt_s and the same substeps");
    if (((int64_t)n_wbin + 1) * ((int64_t)n_rbin + 1) > kHzMaxBin)
        return fail(ctx, "tcr_compound: (n_wbin + 1) * (n_rbin + 1) must be <= 64");
    return 0;
}

template <bool UNIT_C, bool SUM>
hipError_t compound_launch(const CpPrepArgs &p, const tcr_wind_params *wp, const tcr_rain_params *rp, int32_t n_wbin, int32_t n_rbin,
                           double *site_rain, const ScanArgs<CpRec> &m, dim3 grid, size_t lds, hipStream_t st)
{
    const double c = wp->ck_cd, re_km = kWfEarthR / 1000.0;
    return scan_launch(k_compound_prep, p, p.wf.n_trk, m, grid, lds, st,
                       CompoundScan<UNIT_C, SUM>{{c, 2.0 - c, 1.0 / (2.0 - c)}, scan_a_of(wp->r_out_km, re_km),
                                                 scan_a_of(rp->r_out_km, re_km), n_wbin, n_rbin, site_rain});
}

}  // namespace

extern "C" {

int tcr_compound_dev(tcr_ctx *ctx, const tcr_wind_tracks *t, const double *vmax, const tcr_wind_params *wp, const tcr_rain_params *rp,
                     int64_t n_site, const double *site_lon, const double *site_lat, int32_t n_wbin, const double *wthr, int32_t n_rbin,
                     const double *rthr, int32_t *counts, double *site_wind, double *site_rain, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || compound_check(ctx, t, vmax, wp, rp, n_site, site_lon, site_lat, n_wbin, wthr, n_rbin, rthr, counts)) return -1;
    const int64_t n_rec = (t->n_t - 1) * wp->substeps + 1;
    const size_t n_stage = (size_t)std::max<int64_t>(1, t->n_trk * t->n_t);
    double thr[kHzMaxBin] = {};                         // the wind list, then the rain list (n_wbin + n_rbin <= 32)
    for (int b = 0; b < n_wbin; ++b) thr[b] = wthr[b];
    for (int b = 0; b < n_rbin; ++b) thr[n_wbin + b] = rthr[b];
    const tcr_hazard_tracks ht = compound_rain_tracks(t, vmax);
    return scan_run<CpRec>(ctx, ctx->an.cp, "tcr_compound", t, n_rec, n_stage * sizeof(WfStage), n_site, site_lon, site_lat,
                           std::max(wp->r_out_km, rp->r_out_km), kWfEarthR / 1000.0, (n_wbin + 1) * (n_rbin + 1), thr, counts, site_wind,
                           st, [&](const ScanArgs<CpRec> &m, void *stage, dim3 grid, size_t) {
        const size_t lds = sizeof(kJointHist) * 64 * (m.n_bin + 1);      // (the scan zeroes n_bin + 1 rows)
        CpPrepArgs p{};
        p.wf = WfPrepArgs{t->lon, t->lat, t->v, t->u250, t->v250, t->u850, t->v850, t->rmax_km, t->n_trk, t->n_t, t->row_stride,
                          wp->dt_s, wp->rmax_const_km, wp->substeps, static_cast<WfStage *>(stage), ScanRows<WfRec>{}};
        p.rf = RfPrepArgs{ht.lon, ht.lat, ht.vmax, ht.n_trk, ht.n_t, ht.row_stride, rp->dt_s / (3600.0 * rp->substeps), rp->v_lo_kt,
                          rp->v_hi_kt, {rp->a[0], rp->a[1], rp->a[2], rp->a[3]}, {rp->b[0], rp->b[1], rp->b[2], rp->b[3]},
                          rp->substeps, ScanRows<RfRec>{}};
        p.out = m.rows;
        const bool unit = wp->ck_cd == 1.0, sum = rp->stat == TCR_RAIN_TOTAL;
        if (unit && sum) return compound_launch<true, true>(p, wp, rp, n_wbin, n_rbin, site_rain, m, grid, lds, st);
        if (unit) return compound_launch<true, false>(p, wp, rp, n_wbin, n_rbin, site_rain, m, grid, lds, st);
        if (sum) return compound_launch<false, true>(p, wp, rp, n_wbin, n_rbin, site_rain, m, grid, lds, st);
        return compound_launch<false, false>(p, wp, rp, n_wbin, n_rbin, site_rain, m, grid, lds, st);
    }, kJointMaxChunk);
}

int tcr_compound_host(tcr_ctx *ctx, const tcr_wind_tracks *t, const double *vmax, const tcr_wind_params *wp, const tcr_rain_params *rp,
                      int64_t n_site, const double *site_lon, const double *site_lat, int32_t n_wbin, const double *wthr, int32_t n_rbin,
                      const double *rthr, int32_t *counts, double *site_wind, double *site_rain)
{
    if (!enter(ctx) || compound_check(ctx, t, vmax, wp, rp, n_site, site_lon, site_lat, n_wbin, wthr, n_rbin, rthr, counts)) return -1;
    if (!wind_rmax_ok(t)) return fail(ctx, "tcr_compound_host: rmax_km must be finite and > 0 at every sample of a track");
    DevBuf B;
    tcr_wind_tracks d;
    const ScanHostIO io = scan_host_io(B, t, n_site, site_lon, site_lat, (n_wbin + 1) * (n_rbin + 1), site_wind != nullptr);
    const size_t n_plane = (size_t)std::max<int64_t>(1, t->n_trk * t->row_stride);
    const double *d_vmax = t->n_trk > 0 ? B.put(vmax, n_plane) : B.get<double>(1);
    double *d_rain = site_rain ? B.get<double>((size_t)n_site * std::max<int64_t>(1, t->n_trk)) : nullptr;
    if (!wind_tracks_upload(B, t, &d) || !io.ok || !d_vmax || (site_rain && !d_rain))
        return fail(ctx, "tcr_compound_host: device allocation / upload failed");
    if (tcr_compound_dev(ctx, &d, d_vmax, wp, rp, n_site, io.site_lon, io.site_lat, n_wbin, wthr, n_rbin, rthr, io.counts, io.site_max,
                         d_rain, ctx->stream))
        return -1;
    if (site_rain && io.n_max) HIPCHK(ctx, hipMemcpyAsync(site_rain, d_rain, sizeof(double) * io.n_max, hipMemcpyDeviceToHost, ctx->stream));
    return scan_download(ctx, io, counts, site_wind);
}

int tcr_compound_pairs(tcr_ctx *ctx, int64_t *pairs) { return ctx ? scan_pairs(ctx, ctx->an.cp, "tcr_compound", pairs) : -1; }

}  // extern "C"
