// Portfolio loss behind the C ABI (include/tcrisk_hip.h, "portfolio loss" section): what a track ensemble costs a set of exposed
// values, without the site_max[n_site][n_trk] matrix of the wind footprint ever existing.
//
//   m = site_max[i][s]  the footprint peak wind of storm s at site i, exactly tcr_windfield_*'s (NaN: no sample within r_out_km)
//   x = max(m - v_thresh, 0) / (v_half_i - v_thresh),  D = x^3 / (1 + x^3)       Emanuel (2011) damage function; CLIMADA's defaults
//   loss[i][s] = value[i] D                                                       (0 when m is NaN)
//   event_loss[s] = sum_i loss[i][s]     year_agg[g] / year_max[g] = sum / max of event_loss over the storms of group g
//   site_loss[i] = sum_s loss[i][s]      counts: the footprint's exceedance counts, which the scan computes anyway
//
// A user of the site scan (tcr_sitescan.h) with the footprint's own prep kernel, record and value (k_wind_prep, WfRec, WindScan of
// tcr_windfield.hip).  What is the loss's own:
//   LossScan<c == 1>  WindScan with the loss's parameters and buffers, and LossMode for its mode;
//   LossMode          the scan's peak mode plus the loss.  A lane holds value and 1 / (v_half_i - v_thresh) of its site over the
//                     chunk; once a storm's m is known it computes its loss and adds it to its running sum of the chunk's storms
//                     (storm order), which goes to site_part [n_chunk][n_site]; per storm the wave sums its 64 lane losses with a
//                     fixed butterfly and lane 0 stores the sum to tile_loss [n_tile][n_trk] (a storm culled for the whole tile: 0,
//                     without the butterfly);
//   k_loss_events     one thread per storm: event_loss[s] = tile_loss[0][s] + tile_loss[1][s] + ... (coalesced: [tile][storm]);
//   k_loss_years      one wave per group: lane j sums every 64th storm of the group from the j-th on, then the butterfly; the maximum
//                     likewise (a max does not depend on the order);
//   k_loss_sites      one thread per site: the per-chunk site sums in ascending chunk order.
//
// No floating-point atomics: the order of every sum is a function of the inputs (sites -> tiles, group offsets -> chunks), so a
// repeated call is bit-identical.  event_loss[s] does not depend on the other storms of the call at all: tiles are runs of 64 sites
// of the caller's site order, and a tile's sum is the same butterfly whichever chunk the storm is in.

namespace {

struct LossTerms { double value, inv; };    // exposed value (0: contributes nothing) and 1 / (v_half - v_thresh) of a lane's site

// the mode of LossScan: ScanPeak<false> (the footprint's counts), with the loss between the storm's peak and its count
struct LossMode : ScanPeak<false> {
    LossTerms terms;                        // of this lane's site
    double loss_acc = 0.0;                  // this site's losses of the chunk's storms, summed in storm order
    template <class P> __device__ __forceinline__ void begin(const P &pol, const ScanLane &c)
    {
        ScanPeak<false>::begin(pol, c);
        terms = pol.site_terms(c.my, c.valid);
    }
    template <class P> __device__ __forceinline__ void end_storm(const P &pol, const ScanLane &c, const Storm &st, int64_t s, bool near)
    {
        store(c, s, st.m);
        double t = 0.0;                                 // a storm culled for the whole tile: 0, without the butterfly
        if (near) {
            const double l = pol.loss(terms, st.m);
            loss_acc += l;
            t = wave_sum(l);
        }
        if (c.lane == 0) pol.tile_loss[c.tile * c.a.n_trk + s] = t;
        count(c, st.m);
    }
    template <class P> __device__ __forceinline__ void end_chunk(const P &pol, const ScanLane &c)
    {
        ScanPeak<false>::end_chunk(pol, c);
        if (c.valid) pol.site_part[c.chunk * c.a.n_site + c.site] = loss_acc;
    }
};

template <bool UNIT_C>
struct LossScan : WindScan<UNIT_C> {
    using Mode = LossMode;
    const double *site_value, *site_v_half; // [n_site]; site_v_half NULL: v_half0 everywhere
    double v_thresh, v_half0;
    double *tile_loss;                      // [n_tile][n_trk]
    double *site_part;                      // [n_chunk][n_site]
    // a lane without a site, or a site with a bad value (not finite, < 0) or a bad v_half (not finite, <= v_thresh, or so close to
    // it that the reciprocal overflows) contributes 0
    __device__ __forceinline__ LossTerms site_terms(int64_t site, bool valid) const
    {
        const double v = site_value[site], vh = site_v_half ? site_v_half[site] : v_half0;
        const double inv = 1.0 / (vh - v_thresh);
        const bool ok = valid && isfinite(v) && v >= 0.0 && isfinite(vh) && vh > v_thresh && isfinite(inv);
        return ok ? LossTerms{v, inv} : LossTerms{0.0, 0.0};
    }
    __device__ __forceinline__ double loss(const LossTerms &t, double m) const
    {
        const double x = fmax(m - v_thresh, 0.0) * t.inv;       // fmax skips NaN: no wind, no loss
        const double x3 = x * x * x;
        return t.value * (isfinite(x3) ? x3 / (1.0 + x3) : 1.0);
    }
};

__global__ __launch_bounds__(256) void k_loss_events(const double *__restrict__ tile_loss, int64_t n_tile, int64_t n_trk,
                                                     double *__restrict__ event_loss)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_trk) return;
    double sum = 0.0;
    for (int64_t k = 0; k < n_tile; ++k) sum += tile_loss[k * n_trk + s];
    event_loss[s] = sum;
}

// chunks, gch_off: the scan's chunk table; the storms of group g are [begin of its first chunk, end of its last chunk)
__global__ __launch_bounds__(64) void k_loss_years(const double *__restrict__ event_loss, const int64_t *__restrict__ chunks,
                                                   const int64_t *__restrict__ gch_off, double *__restrict__ year_agg,
                                                   double *__restrict__ year_max)
{
    const int64_t g = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t c0 = gch_off[g], c1 = gch_off[g + 1];
    double sum = 0.0, mx = 0.0;
    if (c1 > c0) {
        const int64_t b = chunks[3 * c0], e = chunks[3 * (c1 - 1) + 1];
        for (int64_t s = b + lane; s < e; s += 64) { const double l = event_loss[s]; sum += l; mx = fmax(mx, l); }
    }
    sum = wave_sum(sum); mx = wave_max(mx);
    if (lane == 0) { year_agg[g] = sum; year_max[g] = mx; }
}

__global__ __launch_bounds__(256) void k_loss_sites(const double *__restrict__ site_part, int64_t n_chunk, int64_t n_site,
                                                    double *__restrict__ site_loss)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_site) return;
    double sum = 0.0;
    for (int64_t k = 0; k < n_chunk; ++k) sum += site_part[k * n_site + i];
    site_loss[i] = sum;
}

int loss_check(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *wp, const tcr_loss_params *lp, int64_t n_site,
               const double *site_lon, const double *site_lat, const double *site_value, int32_t n_bin, const double *thr,
               const int32_t *counts, const double *event_loss, const double *year_agg, const double *year_max,
               const double *site_loss)
{
    if (!lp || !site_value || !event_loss || !year_agg || !year_max || !site_loss) return fail(ctx, "tcr_loss: NULL argument");
    if (!(std::isfinite(lp->v_thresh) && lp->v_thresh >= 0.0)) return fail(ctx, "tcr_loss: v_thresh must be finite and >= 0");
    if (!(std::isfinite(lp->v_half) && lp->v_half > lp->v_thresh)) return fail(ctx, "tcr_loss: v_half must be finite and > v_thresh");
    return windfield_check(ctx, t, wp, n_site, site_lon, site_lat, n_bin, thr, counts);
}

}  // namespace

extern "C" {

int tcr_loss_dev(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *prm, const tcr_loss_params *lp, int64_t n_site,
                 const double *site_lon, const double *site_lat, const double *site_value, const double *site_v_half, int32_t n_bin,
                 const double *thresholds, int32_t *counts, double *event_loss, double *year_agg, double *year_max, double *site_loss,
                 void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || loss_check(ctx, t, prm, lp, n_site, site_lon, site_lat, site_value, n_bin, thresholds, counts, event_loss, year_agg,
                          year_max, site_loss))
        return -1;
    ScanWs &w = ctx->an.ls;
    const ScanPlan plan = scan_plan(t, n_site, kScanAnyChunk);
    const int64_t n_trk = t->n_trk, n_tile = plan.n_tile, n_chunk = plan.n_chunk;
    if (n_tile * std::max<int64_t>(1, n_trk) >= ((int64_t)1 << 40) ||
        w.d[kWsOwn0].grow(ctx, sizeof(double) * (size_t)std::max<int64_t>(1, n_tile * n_trk)) < 0 ||
        w.d[kWsOwn1].grow(ctx, sizeof(double) * (size_t)std::max<int64_t>(1, n_chunk * n_site)) < 0) {
        (void)hipGetLastError();
        return fail(ctx, "tcr_loss: the tile-loss workspace (sites / 64 x storms doubles) does not fit; split the sites");
    }
    double *tile_loss = reinterpret_cast<double *>(w.d[kWsOwn0].p), *site_part = reinterpret_cast<double *>(w.d[kWsOwn1].p);
    const int64_t n_rec = (t->n_t - 1) * prm->substeps + 1;
    const size_t n_stage = (size_t)std::max<int64_t>(1, n_trk * t->n_t);
    const int rc = scan_run<WfRec>(ctx, w, "tcr_loss", t, plan, LossMode::shape(n_bin, thresholds), n_rec, n_stage * sizeof(WfStage), n_site,
                                   site_lon, site_lat, prm->r_out_km, kWfEarthR / 1000.0, counts, nullptr, st,
                                   [&](const ScanRows<WfRec> &rows, const ScanLaunch &L, void *stage) {
        if (prm->ck_cd == 1.0)
            return wind_scan_launch(t, prm, rows, L, stage,
                                    LossScan<true>{wind_scan<true>(prm), site_value, site_v_half, lp->v_thresh, lp->v_half, tile_loss, site_part});
        return wind_scan_launch(t, prm, rows, L, stage,
                                LossScan<false>{wind_scan<false>(prm), site_value, site_v_half, lp->v_thresh, lp->v_half, tile_loss, site_part});
    });
    if (rc) return rc;
    const int64_t *d_tab = scan_dev_tab(w);
    if (n_trk > 0)
        hipLaunchKernelGGL(k_loss_events, dim3((unsigned)((n_trk + 255) / 256)), dim3(256), 0, st, tile_loss, n_tile, n_trk, event_loss);
    hipLaunchKernelGGL(k_loss_years, dim3((unsigned)t->n_group), dim3(64), 0, st, event_loss, d_tab, d_tab + plan.tab.size(), year_agg,
                       year_max);
    hipLaunchKernelGGL(k_loss_sites, dim3((unsigned)((n_site + 255) / 256)), dim3(256), 0, st, site_part, n_chunk, n_site, site_loss);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(w.done, st));
    return 0;
}

int tcr_loss_host(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *prm, const tcr_loss_params *lp, int64_t n_site,
                  const double *site_lon, const double *site_lat, const double *site_value, const double *site_v_half, int32_t n_bin,
                  const double *thresholds, int32_t *counts, double *event_loss, double *year_agg, double *year_max, double *site_loss)
{
    if (!enter(ctx) || loss_check(ctx, t, prm, lp, n_site, site_lon, site_lat, site_value, n_bin, thresholds, counts, event_loss, year_agg,
                                  year_max, site_loss))
        return -1;
    // what the device entry point cannot report
    for (int64_t i = 0; i < n_site; ++i) {
        if (!(std::isfinite(site_value[i]) && site_value[i] >= 0.0)) return fail(ctx, "tcr_loss_host: site_value must be finite and >= 0");
        if (site_v_half && !(std::isfinite(site_v_half[i]) && site_v_half[i] > lp->v_thresh))
            return fail(ctx, "tcr_loss_host: site_v_half must be finite and > v_thresh at every site");
    }
    DevBuf B;
    tcr_wind_tracks d;
    const ScanHostIO io = scan_host_io(B, t, n_site, site_lon, site_lat, n_bin, false);
    const double *d_value = B.put(site_value, (size_t)n_site);
    const double *d_vhalf = site_v_half ? B.put(site_v_half, (size_t)n_site) : nullptr;
    double *d_event = B.get<double>((size_t)std::max<int64_t>(1, t->n_trk));
    double *d_agg = B.get<double>((size_t)t->n_group), *d_max = B.get<double>((size_t)t->n_group);
    double *d_site = B.get<double>((size_t)n_site);
    if (!wind_tracks_upload(B, t, &d) || !io.ok || !d_value || (site_v_half && !d_vhalf) || !d_event || !d_agg || !d_max || !d_site)
        return fail(ctx, "tcr_loss_host: device allocation / upload failed");
    if (tcr_loss_dev(ctx, &d, prm, lp, n_site, io.site_lon, io.site_lat, d_value, d_vhalf, n_bin, thresholds, io.counts, d_event, d_agg,
                     d_max, d_site, ctx->stream))
        return -1;
    if (t->n_trk > 0)
        HIPCHK(ctx, hipMemcpyAsync(event_loss, d_event, sizeof(double) * (size_t)t->n_trk, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(year_agg, d_agg, sizeof(double) * (size_t)t->n_group, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(year_max, d_max, sizeof(double) * (size_t)t->n_group, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(site_loss, d_site, sizeof(double) * (size_t)n_site, hipMemcpyDeviceToHost, ctx->stream));
    return scan_download(ctx, io, counts, nullptr);
}

}  // extern "C"
