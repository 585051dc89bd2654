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
// A user of the site scan (tcr_sitescan.h: tiling, culling, counts; its kLevels variant) on the wind footprint's records: the prep
// kernel is k_wind_prep itself, the wind of a pair is WindScan's.  What is the duration's own:
//   DuRec             WfRec read with its half-weight: the one record slot WfRec::uniform leaves alone;
//   DurationScan      the policy of k_site_scan: WindScan's value, the record's half-weight, the levels and where the planes go;
//   k_duration_reduce sums the int64 per-chunk totals of each group.
// No formula is restated here.
//
// Bit-identity: tcr_sitescan.h's argument for kLevels.  Everything accumulated is an integer, so every output is the same bits
// whatever the launch shape, the site order, the storm order and the chunking.  That is what the half-weights are for: a sum of
// fp64 hours would depend on its order, and on the chunking once it crosses storms.

namespace {

constexpr int kDuMaxLevel = kScanMaxLevel;

// a footprint record as the duration scan reads it: the terms WfRec::uniform loads, and hw as the integer k_wind_prep stored
struct DuRec {
    double sp, cp, sl, cl, cosp, sinp, sinl, cosl, rm, mm, f2, a2, be, bn;
    int64_t hw;
    double pad1;
    static __device__ __forceinline__ DuRec uniform(const DuRec *p)
    {
        const double *d = &p->sp;
        return DuRec{hz_uniform(d), hz_uniform(d + 1), hz_uniform(d + 2), hz_uniform(d + 3), hz_uniform(d + 4), hz_uniform(d + 5),
                     hz_uniform(d + 6), hz_uniform(d + 7), hz_uniform(d + 8), hz_uniform(d + 9), hz_uniform(d + 10), hz_uniform(d + 11),
                     hz_uniform(d + 12), hz_uniform(d + 13), hz_uniform(&p->hw), 0.0};
    }
    __device__ __forceinline__ WfRec wind() const { return WfRec{sp, cp, sl, cl, cosp, sinp, sinl, cosl, rm, mm, f2, a2, be, bn, 0.0, 0.0}; }
};
static_assert(sizeof(DuRec) == sizeof(WfRec) && offsetof(DuRec, hw) == offsetof(WfRec, hw) && offsetof(DuRec, bn) == offsetof(WfRec, bn),
              "DuRec is WfRec's layout");

// the policy of k_site_scan<DurationScan<UNIT_C, NL>>: the kLevels variant with NL accumulators (the call's n_level <= NL)
template <bool UNIT_C, int NL>
struct DurationScan {
    using Rec = DuRec;
    static constexpr int kUnroll = 2;
    static constexpr int kLevels = NL;
    WindScan<UNIT_C> wind;
    double level[NL];                       // ascending; +inf past n_level
    double unit;                            // u: hours per half-weight
    int32_t n_level, n_hbin;
    double *site_level[NL];                 // site_hours[l] [n_site][n_trk], or NULL
    int64_t *level_part;                    // [n_chunk][n_site][n_level]
    __device__ __forceinline__ double value(const ScanSite &s, const DuRec &p, double q) const { return wind.value(s, p.wind(), q); }
    __device__ __forceinline__ int32_t weight(const DuRec &p) const { return (int32_t)p.hw; }
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
    if (n_level < 1 || n_level > kDuMaxLevel) return fail(ctx, "tcr_duration: n_level must be in [1, 8]");
    for (int l = 0; l < n_level; ++l)
        if (!std::isfinite(levels[l]) || !(levels[l] > 0.0) || (l > 0 && !(levels[l] > levels[l - 1])))
            return fail(ctx, "tcr_duration: levels must be finite, > 0 and ascending");
    if ((int64_t)n_level * ((int64_t)n_bin + 1) > kHzMaxBin) return fail(ctx, "tcr_duration: n_level * (n_bin + 1) must be <= 64");
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
hipError_t duration_launch(const DuCall &d, const ScanArgs<WfRec> &m, void *stage, dim3 grid, hipStream_t st)
{
    const tcr_wind_tracks *t = d.t;
    const double c = d.prm->ck_cd;
    DurationScan<UNIT_C, NL> pol{};
    pol.wind = WindScan<UNIT_C>{c, 2.0 - c, 1.0 / (2.0 - c)};
    for (int l = 0; l < NL; ++l) {
        pol.level[l] = l < d.n_level ? d.levels[l] : INFINITY;
        pol.site_level[l] = (d.site_hours && l < d.n_level) ? d.site_hours[l] : nullptr;
    }
    pol.unit = d.prm->dt_s / (7200.0 * d.prm->substeps);
    pol.n_level = d.n_level; pol.n_hbin = d.n_bin;
    pol.level_part = d.level_part;
    // the footprint's rows under the duration's view of a record
    ScanArgs<DuRec> v{};
    v.rows = ScanRows<DuRec>{reinterpret_cast<DuRec *>(m.rows.rec), m.rows.seg, m.rows.storm, m.rows.cnt, m.rows.n_seg_max};
    v.chunks = m.chunks; v.site_lon = m.site_lon; v.site_lat = m.site_lat;
    v.n_site = m.n_site; v.n_tile = m.n_tile; v.n_trk = m.n_trk;
    v.a_R = m.a_R; v.r_ang = m.r_ang; v.n_bin = m.n_bin;
    for (int b = 0; b < kHzMaxBin; ++b) v.thr[b] = m.thr[b];
    v.part = m.part; v.site_max = nullptr; v.pairs = m.pairs;
    WfPrepArgs p{t->lon, t->lat, t->v, t->u250, t->v250, t->u850, t->v850, t->rmax_km, t->n_trk, t->n_t, t->row_stride,
                 d.prm->dt_s, d.prm->rmax_const_km, d.prm->substeps, static_cast<WfStage *>(stage), m.rows};
    const size_t lds = sizeof(int32_t) * 64 * (size_t)d.n_level * (d.n_bin + 1);         // (the scan zeroes n_level (n_bin + 1) rows)
    return scan_launch(k_wind_prep, p, t->n_trk, v, grid, lds, st, pol);
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
    const int64_t n_tile = (n_site + 63) / 64;
    std::vector<int64_t> tab, gch;
    scan_chunks(t, n_tile, tab, gch);                   // scan_run's own table: the size of the totals' workspace
    const int64_t n_chunk = (int64_t)tab.size() / 3;
    if (w.d[6].grow(ctx, sizeof(int64_t) * (size_t)std::max<int64_t>(1, n_chunk * n_site * n_level)) < 0) return -1;
    int64_t *level_part = reinterpret_cast<int64_t *>(w.d[6].p);
    const int64_t n_rec = (t->n_t - 1) * prm->substeps + 1;
    const size_t n_stage = (size_t)std::max<int64_t>(1, t->n_trk * t->n_t);
    double thr[kHzMaxBin] = {};                         // the n_bin thresholds; the scan is handed n_level n_bin >= n_bin of these
    for (int b = 0; b < n_bin; ++b) thr[b] = thresholds[b];
    const DuCall d{t, prm, n_level, n_bin, levels, site_hours, level_part};
    const int rc = scan_run<WfRec>(ctx, w, "tcr_duration", t, n_rec, n_stage * sizeof(WfStage), n_site, site_lon, site_lat, prm->r_out_km,
                                   kWfEarthR / 1000.0, n_level * n_bin, thr, counts, nullptr, st,
                                   [&](const ScanArgs<WfRec> &m, void *stage, dim3 grid, size_t) {
        const bool unit = prm->ck_cd == 1.0, few = n_level <= 4;
        if (unit && few) return duration_launch<true, 4>(d, m, stage, grid, st);
        if (unit) return duration_launch<true, kDuMaxLevel>(d, m, stage, grid, st);
        if (few) return duration_launch<false, 4>(d, m, stage, grid, st);
        return duration_launch<false, kDuMaxLevel>(d, m, stage, grid, st);
    });
    if (rc) return rc;
    if (half_steps) {
        const int64_t n_out = n_site * t->n_group * n_level;
        hipLaunchKernelGGL(k_duration_reduce, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, level_part,
                           reinterpret_cast<const int64_t *>(w.d[4].p) + tab.size(), n_site, t->n_group, n_level, half_steps);
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
    const size_t n_half = (size_t)n_site * t->n_group * n_level, n_plane = (size_t)n_site * std::max<int64_t>(1, t->n_trk);
    int64_t *d_half = half_steps ? B.get<int64_t>(n_half) : nullptr;
    double *d_hours[kDuMaxLevel] = {};
    bool ok = wind_tracks_upload(B, t, &d) && io.ok && (!half_steps || d_half);
    for (int l = 0; l < n_level && ok; ++l)
        if (site_hours && site_hours[l]) ok = (d_hours[l] = B.get<double>(n_plane)) != nullptr;
    if (!ok) return fail(ctx, "tcr_duration_host: device allocation / upload failed");
    if (tcr_duration_dev(ctx, &d, prm, n_site, io.site_lon, io.site_lat, n_level, levels, n_bin, thresholds, io.counts, d_half, d_hours,
                         ctx->stream))
        return -1;
    if (half_steps) HIPCHK(ctx, hipMemcpyAsync(half_steps, d_half, sizeof(int64_t) * n_half, hipMemcpyDeviceToHost, ctx->stream));
    for (int l = 0; l < n_level; ++l)
        if (d_hours[l] && io.n_max)
            HIPCHK(ctx, hipMemcpyAsync(site_hours[l], d_hours[l], sizeof(double) * io.n_max, hipMemcpyDeviceToHost, ctx->stream));
    return scan_download(ctx, io, counts, nullptr);
}

int tcr_duration_pairs(tcr_ctx *ctx, int64_t *pairs) { return ctx ? scan_pairs(ctx, ctx->an.du, "tcr_duration", pairs) : -1; }

}  // extern "C"
