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
// A user of the site scan (tcr_sitescan.h: tiling, culling, the mode protocol).  What is the compound's own:
//   CpRec             one sample or sub-sample (160 bytes): the position terms once, then the wind terms of WfRec and the rain
//                     terms of RfRec;
//   k_compound_prep   one wave per storm: finds the track over the eight planes (ballot), stages the footprint's per-sample terms
//                     (wf_stage), then writes one record per sample and sub-sample: wf_sub_record and rf_sub_record side by side;
//   CompoundScan      the policy of k_site_scan: WindScan's value under the wind radius, RainScan's under the rain radius, on the
//                     one angle ScanJoint forms per included pair;
//   ScanJoint<SUM>    the mode: two hazards of one record at once.  The scan includes a pair under the larger radius (a_R and r_ang,
//                     the culling, are that radius's); the pair's angle is formed once; first(site, record, angle) goes into a max
//                     under the policy's a_first and second(site, record, angle) into a max, or with SUM into a sum in record
//                     order, under its a_second.  site_max takes the first, the policy's site_second the second.  thr holds the
//                     n_first thresholds of the first, then the n_second of the second, and the histogram is two-dimensional:
//                     n_cell = (n_first + 1) (n_second + 1) and counts[site][group][a (n_second + 1) + b] = #storms of the group
//                     passing at least a thresholds of the first and at least b of the second (a NaN passes none, so index 0 is
//                     "no condition" and [0][0] the size of the group).
//                     A wave's histogram is its LDS, and 64 cells of int32 per lane (16 KB) leave room for 9 waves on a CU: the
//                     joint scan ran at 2 waves / SIMD and 1.6 x slower than with 9 cells (profiles/compound_bench.txt).  So its
//                     cells are kJointHist (16 bits), and the plan keeps a chunk at kJointMaxChunk storms or fewer, which no cell
//                     and no suffix sum can exceed.
// No formula is restated here: records, interpolation and per-pair values are the footprint's and the rainfall's own functions.
//
// Bit-identity.  Each of ScanJoint's two accumulators sees exactly the records with a <= its own a threshold, in record order, and
// nothing else: the cull uses the larger radius, so it is conservative for both; the test of one hazard never gates the other; the
// values come from the functions the single-hazard policies call, on the same record terms and the same angle expression.  So each
// plane is bit for bit what the single-hazard scan of that policy writes (tcr_sitescan.h: one lane, one accumulator), and the 2-D
// counts are integer sums of per-storm ranks of those values.  A record's position terms are the same bits in wf_sub_record and
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
    __device__ __forceinline__ WfRec wind() const { return WfRec{sp, cp, sl, cl, cosp, sinp, sinl, cosl, wrm, mm, f2, a2, be, bn, 0, 0.0}; }
    __device__ __forceinline__ RfRec rain() const { return RfRec{sp, cp, sl, cl, cosp, t0, slope, tm, rrm, ire, w, sinp, sinl, cosl, 0, 0}; }
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

using kJointHist = uint16_t;                // a cell of the joint scan's LDS histogram
constexpr int64_t kJointMaxChunk = 65535;   // storms of a chunk it can count

// the mode of CompoundScan (header comment); cells [n_first + 1][n_second + 1][64] of kJointHist: the storms of this lane passing
// exactly (kw, kr) thresholds of each list
template <bool SUM>
struct ScanJoint {
    struct Storm { double m = NAN, m2 = NAN; };
    // thr: the first list, then the second (n_first + n_second of them)
    static ScanShape shape(int32_t n_first, int32_t n_second, const double *thr)
    {
        const int32_t n_cell = (n_first + 1) * (n_second + 1);
        return ScanShape{n_cell, sizeof(kJointHist) * 64 * (n_cell + 1), n_first + n_second, thr};      // (begin zeroes n_cell + 1 cells)
    }
    template <class P> __device__ __forceinline__ void begin(const P &, const ScanLane &c)
    {
        kJointHist *hist = reinterpret_cast<kJointHist *>(c.lds);
        for (int k = 0; k <= c.a.n_cell; ++k) hist[k * 64 + c.lane] = 0;
    }
    template <class P, class Rec> __device__ __forceinline__ void add(const P &pol, Storm &st, const ScanSite &me, const Rec &p, double q)
    {
        const double ang = scan_pair_angle(q);          // q <= a_R, the larger radius; then each hazard under its own
        if (q <= pol.a_first) st.m = fmax(st.m, pol.first(me, p, ang));
        if (q <= pol.a_second) {
            const double v = pol.second(me, p, ang);
            if constexpr (SUM) st.m2 = isnan(st.m2) ? v : st.m2 + v;            // in record order
            else st.m2 = fmax(st.m2, v);
        }
    }
    template <class P> __device__ __forceinline__ void end_storm(const P &pol, const ScanLane &c, const Storm &st, int64_t s, bool)
    {
        kJointHist *hist = reinterpret_cast<kJointHist *>(c.lds);
        if (c.a.site_max && c.valid) c.a.site_max[c.site * c.a.n_trk + s] = st.m;
        if (pol.site_second && c.valid) pol.site_second[c.site * c.a.n_trk + s] = st.m2;
        // every storm is counted: a NaN has rank 0
        const int kw = scan_rank(c.a.thr, pol.n_first, st.m), kr = scan_rank(c.a.thr + pol.n_first, pol.n_second, st.m2);
        hist[(kw * (pol.n_second + 1) + kr) * 64 + c.lane] += 1;
    }
    template <class P> __device__ __forceinline__ void end_chunk(const P &pol, const ScanLane &c)
    {
        kJointHist *hist = reinterpret_cast<kJointHist *>(c.lds);
        const int lane = c.lane;
        // exactly (kw, kr) -> at least (kw, kr): suffix sums along the second axis, then along the first, in the lane's own column
        const int nw = pol.n_first, nr = pol.n_second;
        for (int kw = nw; kw >= 0; --kw)
            for (int kr = nr - 1; kr >= 0; --kr) hist[(kw * (nr + 1) + kr) * 64 + lane] += hist[(kw * (nr + 1) + kr + 1) * 64 + lane];
        for (int kw = nw - 1; kw >= 0; --kw)
            for (int kr = nr; kr >= 0; --kr) hist[(kw * (nr + 1) + kr) * 64 + lane] += hist[((kw + 1) * (nr + 1) + kr) * 64 + lane];
        if (!c.valid) return;
        int32_t *out = c.a.part + (c.chunk * c.a.n_site + c.site) * c.a.n_cell;
        for (int b = 0; b < c.a.n_cell; ++b) out[b] = hist[b * 64 + lane];
    }
};

// the policy of k_site_scan<CompoundScan<UNIT_C, SUM>>: the footprint's wind first and the rainfall's value (SUM: the storm total,
// otherwise the peak rate) second
template <bool UNIT_C, bool SUM>
struct CompoundScan {
    using Rec = CpRec;
    using Mode = ScanJoint<SUM>;
    static constexpr int kUnroll = 2;
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
                           double *site_rain, const ScanLaunch &L)
{
    const double re_km = kWfEarthR / 1000.0;
    return scan_launch(k_compound_prep, p, p.out, L,
                       CompoundScan<UNIT_C, SUM>{wind_scan<UNIT_C>(wp), scan_a_of(wp->r_out_km, re_km), scan_a_of(rp->r_out_km, re_km),
                                                 n_wbin, n_rbin, site_rain});
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
    double thr[kHzMaxBin];                              // the wind list, then the rain list (n_wbin + n_rbin <= 32)
    for (int b = 0; b < n_wbin; ++b) thr[b] = wthr[b];
    for (int b = 0; b < n_rbin; ++b) thr[n_wbin + b] = rthr[b];
    const tcr_hazard_tracks ht = compound_rain_tracks(t, vmax);
    // (both stats' modes have the one shape)
    return scan_run<CpRec>(ctx, ctx->an.cp, "tcr_compound", t, scan_plan(t, n_site, kJointMaxChunk), ScanJoint<true>::shape(n_wbin, n_rbin, thr),
                           n_rec, n_stage * sizeof(WfStage), n_site, site_lon, site_lat, std::max(wp->r_out_km, rp->r_out_km),
                           kWfEarthR / 1000.0, counts, site_wind, st, [&](const ScanRows<CpRec> &rows, const ScanLaunch &L, void *stage) {
        const CpPrepArgs p{wind_prep_args(t, wp, stage, ScanRows<WfRec>{}), rain_prep_args(&ht, rp, ScanRows<RfRec>{}), rows};
        const bool unit = wp->ck_cd == 1.0, sum = rp->stat == TCR_RAIN_TOTAL;
        if (unit && sum) return compound_launch<true, true>(p, wp, rp, n_wbin, n_rbin, site_rain, L);
        if (unit) return compound_launch<true, false>(p, wp, rp, n_wbin, n_rbin, site_rain, L);
        if (sum) return compound_launch<false, true>(p, wp, rp, n_wbin, n_rbin, site_rain, L);
        return compound_launch<false, false>(p, wp, rp, n_wbin, n_rbin, site_rain, L);
    });
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
    double *d_rain = nullptr;
    if (!scan_host_planes(B, io, 1, &site_rain, &d_rain) || !wind_tracks_upload(B, t, &d) || !io.ok || !d_vmax)
        return fail(ctx, "tcr_compound_host: device allocation / upload failed");
    if (tcr_compound_dev(ctx, &d, d_vmax, wp, rp, n_site, io.site_lon, io.site_lat, n_wbin, wthr, n_rbin, rthr, io.counts, io.site_max,
                         d_rain, ctx->stream))
        return -1;
    if (scan_download_planes(ctx, io, 1, &site_rain, &d_rain)) return -1;
    return scan_download(ctx, io, counts, site_wind);
}

int tcr_compound_pairs(tcr_ctx *ctx, int64_t *pairs) { return ctx ? scan_pairs(ctx, ctx->an.cp, "tcr_compound", pairs) : -1; }

}  // extern "C"
