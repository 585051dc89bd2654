// Wind duration behind the C ABI (include/tcrisk_hip.h, "wind duration" section): for how long every storm brings every site a
// footprint wind of at least each of up to eight levels, how many storms do so for at least each of a list of durations, and the
// total time per group, from one scan of the ensemble.
//
//   H[l][site][storm]           = sum of the half-weights h_q (2; 1 for a track's first and last record: the trapezoid rule in units
//                                 of half a sub-step) over the included records whose wind is >= level[l]              (int32)
//   site_hours[l][site][storm]  = (double)H u,  u = dt_s / (7200 substeps) hours; NaN when no record of the storm is included
//   counts[site][group][l][b]   = #storms of the group with site_hours >= thresholds[b]
//   half_steps[site][group][l]  = sum of H over the storms of the group                                                 (int64)
//
// A user of the site scan (tcr_sitescan.h: tiling, culling, the mode protocol) on the wind footprint's records: the prep kernel is
// k_wind_prep itself, the wind of a pair is WindScan's.  What is the duration's own:
//   DurationScan      the policy of k_site_scan: WindScan's value, the record's half-weight (WfRec::hw), the levels and where the
//                     planes go;
//   ScanLevels<NL>    the mode (1 <= NL <= kScanMaxRow): time instead of a peak.  value(site, record, a) is formed once per
//                     included pair and compared with the policy's NL ascending level[] (unused ones +inf), and the record's
//                     integer weight(record) is added to the int32 accumulator of every level the value reaches (>=) and to one
//                     more that counts the included records.  The NL + 1 accumulators are registers: fixed arrays, fully unrolled,
//                     never indexed by a run-time value.  Per storm each of the call's n_row levels has the value
//                     (double)sum * unit (NaN when no record was included): a row of the stacked histogram (ScanStack,
//                     tcr_sitescan.h: the plane, the rank, the partial counts).  Every lane also keeps an int64 total of its sums
//                     per level over the chunk's storms and writes it to the policy's level_part [n_chunk][n_site][n_level].
//                     There is no max: the call's site_max is NULL and nothing reads it;
//   k_duration_reduce sums the int64 per-chunk totals of each group.
// No formula is restated here.
//
// Bit-identity, by the scan's first argument alone (tcr_sitescan.h): everything ScanLevels accumulates is an integer.  A pair's
// value and weight do not depend on the other pairs, a skipped pair is never an included one, and int32 and int64 sums do not
// depend on order; the value written is one conversion and one multiply of such a sum.  So every output is the same bits whatever
// the launch shape, the site order, the storm order and the chunking.  That is what the half-weights are for: a sum of fp64 hours
// would depend on its order, and on the chunking once it crosses storms.

namespace {

// the mode of DurationScan (header comment), on ScanStack with the levels for rows
template <int NL>
struct ScanLevels {
    struct Storm {
        int32_t lv[NL] = {};                // the weights of the records that reach each level,
        int32_t lv_in = 0;                  // and of every included record
    };
    int64_t lv_total[NL] = {};              // this site's sums of the chunk's storms, per level
    template <class P> __device__ __forceinline__ void begin(const P &pol, const ScanLane &c) { ScanStack::begin(c, pol.out.n_row, pol.out.n_hbin); }
    template <class P, class Rec> __device__ __forceinline__ void add(const P &pol, Storm &st, const ScanSite &me, const Rec &p, double q)
    {
        const double v = pol.value(me, p, q);
        const int32_t h = pol.weight(p);
        st.lv_in += h;
#pragma unroll
        for (int l = 0; l < NL; ++l) st.lv[l] += v >= pol.level[l] ? h : 0;               // (a NaN reaches none)
    }
    // a row per level; a storm without an included record counts nowhere
    template <class P> __device__ __forceinline__ void end_storm(const P &pol, const ScanLane &c, const Storm &st, int64_t s, bool)
    {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l < pol.out.n_row) {                    // (wave-uniform)
                ScanStack::finish(pol.out, c, l, s, st.lv_in != 0, st.lv_in ? (double)st.lv[l] * pol.unit : NAN);
                lv_total[l] += st.lv[l];
            }
        }
    }
    // the rows' partial counts; and the level's total
    template <class P> __device__ __forceinline__ void end_chunk(const P &pol, const ScanLane &c)
    {
        ScanStack::end_chunk(c, pol.out.n_row, pol.out.n_hbin);
        if (!c.valid) return;
#pragma unroll
        for (int l = 0; l < NL; ++l)
            if (l < pol.out.n_row) pol.level_part[(c.chunk * c.a.n_site + c.site) * pol.out.n_row + l] = lv_total[l];
    }
};

// the policy of k_site_scan<DurationScan<UNIT_C, NL>>: NL accumulators (the call's n_level <= NL)
template <bool UNIT_C, int NL>
struct DurationScan {
    using Rec = WfRec;
    using Mode = ScanLevels<NL>;
    static constexpr int kUnroll = 2;
    WindScan<UNIT_C> wind;
    double level[NL];                       // ascending; +inf past n_level
    double unit;                            // u: hours per half-weight
    ScanStackOut<NL> out;                   // n_level rows; the planes are site_hours[l]
    int64_t *level_part;                    // [n_chunk][n_site][n_level]
    __device__ __forceinline__ double value(const ScanSite &s, const WfRec &p, double q) const { return wind.value(s, p, q); }
    __device__ __forceinline__ int32_t weight(const WfRec &p) const { return (int32_t)p.hw; }
};

// half_steps[site][g][l] = sum of the totals of the chunks of group g
__global__ __launch_bounds__(256) void k_duration_reduce(const int64_t *__restrict__ part, const int64_t *__restrict__ gch_off,
                                                         int64_t n_site, int32_t n_group, int32_t n_level, int64_t *__restrict__ half_steps)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_site * n_group * n_level) return;
    const int64_t l = i % n_level, g = (i / n_level) % n_group, site = i / ((int64_t)n_level * n_group);
    int64_t c = 0;
    for (int64_t k = gch_off[g]; k < gch_off[g + 1]; ++k) c += part[(k * n_site + site) * n_level + l];
    half_steps[i] = c;
}

int duration_check(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *p, int64_t n_site, const double *site_lon,
                   const double *site_lat, int32_t n_level, const double *levels, int32_t n_bin, const double *thr, const int32_t *counts)
{
    if (!levels) return fail(ctx, "tcr_duration: NULL argument");
    if (windfield_check(ctx, t, p, n_site, site_lon, site_lat, n_bin, thr, counts, "tcr_duration")) return -1;
    if (!(thr[0] > 0.0)) return fail(ctx, "tcr_duration: thresholds must be > 0");
    if (scan_stack_check(ctx, "tcr_duration", "level", n_level, n_bin)) return -1;
    for (int l = 0; l < n_level; ++l)
        if (!std::isfinite(levels[l]) || !(levels[l] > 0.0) || (l > 0 && !(levels[l] > levels[l - 1])))
            return fail(ctx, "tcr_duration: levels must be finite, > 0 and ascending");
    return 0;
}

struct DuCall {
    const tcr_wind_tracks *t;
    const tcr_wind_params *prm;
    int32_t n_level, n_bin;
    const double *levels;
    double *const *site_hours;
    int64_t *level_part;
};

template <bool UNIT_C, int NL>
hipError_t duration_launch(const DuCall &d, const ScanRows<WfRec> &rows, const ScanLaunch &L, void *stage)
{
    DurationScan<UNIT_C, NL> pol{};
    pol.wind = wind_scan<UNIT_C>(d.prm);
    for (int l = 0; l < NL; ++l) {
        pol.level[l] = l < d.n_level ? d.levels[l] : INFINITY;
        pol.out.plane[l] = (d.site_hours && l < d.n_level) ? d.site_hours[l] : nullptr;
    }
    pol.unit = d.prm->dt_s / (7200.0 * d.prm->substeps);
    pol.out.n_row = d.n_level; pol.out.n_hbin = d.n_bin;
    pol.level_part = d.level_part;
    return wind_scan_launch(d.t, d.prm, rows, L, stage, pol);
}

}  // namespace

extern "C" {

int tcr_duration_dev(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                     const double *site_lat, int32_t n_level, const double *levels, int32_t n_bin, const double *thresholds,
                     int32_t *counts, int64_t *half_steps, double *const *site_hours, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || duration_check(ctx, t, prm, n_site, site_lon, site_lat, n_level, levels, n_bin, thresholds, counts)) return -1;
    ScanWs &w = ctx->an.du;
    const ScanPlan plan = scan_plan(t, n_site, kScanAnyChunk);
    if (w.d[kWsOwn0].grow(ctx, sizeof(int64_t) * (size_t)std::max<int64_t>(1, plan.n_chunk * n_site * n_level)) < 0) return -1;
    int64_t *level_part = reinterpret_cast<int64_t *>(w.d[kWsOwn0].p);
    const int64_t n_rec = (t->n_t - 1) * prm->substeps + 1;
    const size_t n_stage = (size_t)std::max<int64_t>(1, t->n_trk * t->n_t);
    const DuCall d{t, prm, n_level, n_bin, levels, site_hours, level_part};
    const int rc = scan_run<WfRec>(ctx, w, "tcr_duration", t, plan, ScanStack::shape(n_level, n_bin, 0, thresholds), n_rec,
                                   n_stage * sizeof(WfStage), n_site, site_lon, site_lat, prm->r_out_km, kWfEarthR / 1000.0, counts, nullptr,
                                   st, [&](const ScanRows<WfRec> &rows, const ScanLaunch &L, void *stage) {
        const bool unit = prm->ck_cd == 1.0, few = n_level <= 4;
        if (unit && few) return duration_launch<true, 4>(d, rows, L, stage);
        if (unit) return duration_launch<true, kScanMaxRow>(d, rows, L, stage);
        if (few) return duration_launch<false, 4>(d, rows, L, stage);
        return duration_launch<false, kScanMaxRow>(d, rows, L, stage);
    });
    if (rc) return rc;
    if (half_steps) {
        const int64_t n_out = n_site * t->n_group * n_level;
        hipLaunchKernelGGL(k_duration_reduce, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, level_part,
                           scan_dev_tab(w) + plan.tab.size(), n_site, t->n_group, n_level, half_steps);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(w.done, st));
    }
    return 0;
}

int tcr_duration_host(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                      const double *site_lat, int32_t n_level, const double *levels, int32_t n_bin, const double *thresholds,
                      int32_t *counts, int64_t *half_steps, double *const *site_hours)
{
    if (!enter(ctx) || duration_check(ctx, t, prm, n_site, site_lon, site_lat, n_level, levels, n_bin, thresholds, counts)) return -1;
    if (!wind_rmax_ok(t)) return fail(ctx, "tcr_duration_host: rmax_km must be finite and > 0 at every sample of a track");
    DevBuf B;
    tcr_wind_tracks d;
    const ScanHostIO io = scan_host_io(B, t, n_site, site_lon, site_lat, n_level * n_bin, false);
    const size_t n_half = (size_t)n_site * t->n_group * n_level;
    int64_t *d_half = half_steps ? B.get<int64_t>(n_half) : nullptr;
    double *d_hours[kScanMaxRow] = {};
    if (!wind_tracks_upload(B, t, &d) || !io.ok || (half_steps && !d_half) || !scan_host_planes(B, io, n_level, site_hours, d_hours))
        return fail(ctx, "tcr_duration_host: device allocation / upload failed");
    if (tcr_duration_dev(ctx, &d, prm, n_site, io.site_lon, io.site_lat, n_level, levels, n_bin, thresholds, io.counts, d_half, d_hours,
                         ctx->stream))
        return -1;
    if (half_steps) HIPCHK(ctx, hipMemcpyAsync(half_steps, d_half, sizeof(int64_t) * n_half, hipMemcpyDeviceToHost, ctx->stream));
    if (scan_download_planes(ctx, io, n_level, site_hours, d_hours)) return -1;
    return scan_download(ctx, io, counts, nullptr);
}

int tcr_duration_pairs(tcr_ctx *ctx, int64_t *pairs) { return ctx ? scan_pairs(ctx, ctx->an.du, "tcr_duration", pairs) : -1; }

}  // extern "C"
