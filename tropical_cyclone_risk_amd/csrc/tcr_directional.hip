// Directional wind behind the C ABI (include/tcrisk_hip.h, "directional wind" section): the peak footprint wind every storm brings
// every site from each of up to eight equal compass sectors, and how many storms of a group bring at least each of a list of
// speeds from each sector, from one scan of the ensemble.
//
//   w, theta                     of an included (site, record) pair: the footprint's wind vector V (g_e, g_n), its length |w| (the
//                                footprint's double) and the bearing theta of (-w_e, -w_n), the direction it blows from
//   sector k                     theta - sector0_deg in [(k - 1/2) W, (k + 1/2) W) mod 360, W = 360 / n_sector
//   site_dir_max[k][site][storm] = max(0, max of |w| over the storm's included pairs of sector k); NaN when none is included
//   counts[site][group][k][bin]  = #storms of the group with site_dir_max[k] >= thresholds[bin]
//
// A user of the site scan (tcr_sitescan.h: tiling, culling, the mode protocol) on the wind footprint's records: the prep kernel is
// k_wind_prep itself, the wind of a pair is WindScan's (from_angle: at_angle's speed, and the direction).  What is its own:
//   DirectionalScan   the policy of k_site_scan: WindScan, the sector boundaries and where the planes go;
//   ScanSectors<NS>   the mode (1 <= n_sector <= NS <= kScanMaxRow) on ScanStack, a row per sector: a max per sector instead of
//                     one.  The pair's wind and sector are formed once; the NS maxima are registers: a fixed array, fully unrolled,
//                     updated through `k == sec` selects and never indexed by a run-time value.  They start at 0.0 and only a
//                     greater wind replaces one, so a pair without wind (|w| == 0: no sector) changes nothing whichever select it
//                     falls under, and a sector no wind came from ends at 0.0.  There is no site_max: the call's is NULL.
//
// The sector, without per-lane trigonometry.  With F = (fe, fn) a positive multiple of (-w_e, -w_n) and the n_sector boundaries as
// unit vectors b_k = (sin beta_k, cos beta_k), beta_k = sector0_deg + (k - 1/2) W, the sign of the cross product
// s_k = [fe b_k.n >= fn b_k.e] says that theta is at most half a turn clockwise of boundary k.  The policy holds one launch-uniform
// double per boundary, the slope t_k = b_k.e / b_k.n, a scalar operand, and the bits `flip` of the boundaries with b_k.n < 0:
// s_k = [fe >= fn t_k], inverted where the division by b_k.n turned the inequality round: one multiply and one compare per
// boundary and one exclusive-or for all (two doubles per boundary are 32 SGPRs next to the two records in flight, more than the
// scalar file holds: profiles/directional_boundary_ab.txt).  Inverting [>=] gives [<]
// where [<=] is meant, and a slope can be infinite: both only matter for F along a boundary, which rounding decides anyway.
// Going round the boundaries the s_k are one run of ones and one of zeros, and theta lies in the sector behind whose lower boundary
// the run of ones ends: the one k with s_k and not s_k+1 (cyclic).  A rounded sign can only be wrong for a boundary along F, which
// is an end of its run, so the run stays one run and every pair gets exactly one sector: the highest k >= 1 with s_k and not
// s_k+1, else 0.  That default also makes n_sector = 1 (everything) and n_sector = 2 (s_1 and not s_0) total.  The boundary slots
// past n_sector repeat boundary 0, so that slot n_sector - 1 is compared with boundary 0 and the slots behind it with themselves
// (never a sector).  That is NS half-plane tests per included pair next to the asin, the square roots and the divisions the pair
// already pays; an atan2 and a floor per pair would cost more and put a rounded quotient where this has the sign of a difference.
//
// Bit-identity, by the scan's first argument alone (tcr_sitescan.h): a pair's wind and sector do not depend on the other pairs, a
// skipped pair is never an included one, and a max does not depend on order.  No cross-lane or cross-chunk arithmetic.

namespace {

// the mode of DirectionalScan (header comment), on ScanStack with the sectors for rows
template <int NS>
struct ScanSectors {
    struct Storm {
        double m[NS] = {};                  // the peak from each sector, from 0.0
        bool any = false;                   // a record of the storm is included
    };
    template <class P> __device__ __forceinline__ void begin(const P &pol, const ScanLane &c) { ScanStack::begin(c, pol.out.n_row, pol.out.n_hbin); }
    template <class P, class Rec> __device__ __forceinline__ void add(const P &pol, Storm &st, const ScanSite &me, const Rec &p, double q)
    {
        int sec;
        const double w = pol.value(me, p, q, sec);
        st.any = true;
#pragma unroll
        for (int k = 0; k < NS; ++k) st.m[k] = k == sec && w > st.m[k] ? w : st.m[k];     // (a NaN and 0.0 change nothing)
    }
    template <class P> __device__ __forceinline__ void end_storm(const P &pol, const ScanLane &c, const Storm &st, int64_t s, bool)
    {
#pragma unroll
        for (int k = 0; k < NS; ++k)
            if (k < pol.out.n_row) ScanStack::finish(pol.out, c, k, s, st.any, st.any ? st.m[k] : NAN);     // (wave-uniform)
    }
    template <class P> __device__ __forceinline__ void end_chunk(const P &pol, const ScanLane &c) { ScanStack::end_chunk(c, pol.out.n_row, pol.out.n_hbin); }
};

// the policy of k_site_scan<DirectionalScan<UNIT_C, NS>>: NS accumulators (the call's n_sector <= NS)
template <bool UNIT_C, int NS>
struct DirectionalScan {
    using Rec = WfRec;
    using Mode = ScanSectors<NS>;
    static constexpr int kUnroll = 2;
    WindScan<UNIT_C> wind;
    double t[NS];                           // the boundaries' slopes b_k.e / b_k.n; boundary 0 again past n_sector
    unsigned flip;                          // bit k: b_k.n < 0
    ScanStackOut<NS> out;                   // n_sector rows; the planes are site_dir_max[k]
    // the sector of a wind from direction (fe, fn) (header comment)
    __device__ __forceinline__ int sector(double fe, double fn) const
    {
        unsigned s = 0;                     // bit k: s_k.  One register per lane, where NS flags would be NS lane masks (SGPR pairs)
#pragma unroll
        for (int k = 0; k < NS; ++k) s |= fe >= fn * t[k] ? 1u << k : 0u;
        s ^= flip;
        const unsigned next = (s >> 1) | (s << (NS - 1));                   // bit k: s_k+1, cyclic
        const unsigned in = s & ~next & ((1u << NS) - 2u);                   // bit k >= 1: s_k and not s_k+1
        return in ? 31 - __clz((int)in) : 0;
    }
    // |w| of the pair, the footprint's double, and its sector
    __device__ __forceinline__ double value(const ScanSite &s, const WfRec &p, double q, int &sec) const
    {
        double fe, fn;
        const double w = wind.from_angle(s, p, scan_pair_angle(q), fe, fn);
        sec = sector(fe, fn);
        return w;
    }
};

int directional_check(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *p, int64_t n_site, const double *site_lon,
                      const double *site_lat, int32_t n_sector, double sector0_deg, int32_t n_bin, const double *thr, const int32_t *counts)
{
    if (windfield_check(ctx, t, p, n_site, site_lon, site_lat, n_bin, thr, counts, "tcr_directional")) return -1;
    if (scan_stack_check(ctx, "tcr_directional", "sector", n_sector, n_bin)) return -1;
    if (!(std::isfinite(sector0_deg) && sector0_deg >= 0.0 && sector0_deg < 360.0))
        return fail(ctx, "tcr_directional: sector0_deg must be finite and in [0, 360)");
    return 0;
}

struct DrCall {
    const tcr_wind_tracks *t;
    const tcr_wind_params *prm;
    int32_t n_sector, n_bin;
    double sector0_deg;
    double *const *site_dir_max;
};

template <bool UNIT_C, int NS>
hipError_t directional_launch(const DrCall &d, const ScanRows<WfRec> &rows, const ScanLaunch &L, void *stage)
{
    DirectionalScan<UNIT_C, NS> pol{};
    pol.wind = wind_scan<UNIT_C>(d.prm);
    const double width = 360.0 / d.n_sector;
    for (int k = 0; k < NS; ++k) {
        const double beta = (d.sector0_deg + ((k < d.n_sector ? k : 0) - 0.5) * width) * (kPi / 180.0);
        pol.t[k] = sin(beta) / cos(beta);
        pol.flip |= cos(beta) < 0.0 ? 1u << k : 0u;
        pol.out.plane[k] = (d.site_dir_max && k < d.n_sector) ? d.site_dir_max[k] : nullptr;
    }
    pol.out.n_row = d.n_sector; pol.out.n_hbin = d.n_bin;
    return wind_scan_launch(d.t, d.prm, rows, L, stage, pol);
}

}  // namespace

extern "C" {

int tcr_directional_dev(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                        const double *site_lat, int32_t n_sector, double sector0_deg, int32_t n_bin, const double *thresholds,
                        int32_t *counts, double *const *site_dir_max, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || directional_check(ctx, t, prm, n_site, site_lon, site_lat, n_sector, sector0_deg, n_bin, thresholds, counts)) return -1;
    const int64_t n_rec = (t->n_t - 1) * prm->substeps + 1;
    const size_t n_stage = (size_t)std::max<int64_t>(1, t->n_trk * t->n_t);
    const DrCall d{t, prm, n_sector, n_bin, sector0_deg, site_dir_max};
    return scan_run<WfRec>(ctx, ctx->an.dr, "tcr_directional", t, scan_plan(t, n_site, kScanAnyChunk),
                           ScanStack::shape(n_sector, n_bin, 0, thresholds), n_rec, n_stage * sizeof(WfStage), n_site, site_lon, site_lat,
                           prm->r_out_km, kWfEarthR / 1000.0, counts, nullptr, st,
                           [&](const ScanRows<WfRec> &rows, const ScanLaunch &L, void *stage) {
        const bool unit = prm->ck_cd == 1.0, few = n_sector <= 4;
        if (unit && few) return directional_launch<true, 4>(d, rows, L, stage);
        if (unit) return directional_launch<true, kScanMaxRow>(d, rows, L, stage);
        if (few) return directional_launch<false, 4>(d, rows, L, stage);
        return directional_launch<false, kScanMaxRow>(d, rows, L, stage);
    });
}

int tcr_directional_host(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                         const double *site_lat, int32_t n_sector, double sector0_deg, int32_t n_bin, const double *thresholds,
                         int32_t *counts, double *const *site_dir_max)
{
    if (!enter(ctx) || directional_check(ctx, t, prm, n_site, site_lon, site_lat, n_sector, sector0_deg, n_bin, thresholds, counts))
        return -1;
    if (!wind_rmax_ok(t)) return fail(ctx, "tcr_directional_host: rmax_km must be finite and > 0 at every sample of a track");
    DevBuf B;
    tcr_wind_tracks d;
    const ScanHostIO io = scan_host_io(B, t, n_site, site_lon, site_lat, n_sector * n_bin, false);
    double *d_max[kScanMaxRow] = {};
    if (!wind_tracks_upload(B, t, &d) || !io.ok || !scan_host_planes(B, io, n_sector, site_dir_max, d_max))
        return fail(ctx, "tcr_directional_host: device allocation / upload failed");
    if (tcr_directional_dev(ctx, &d, prm, n_site, io.site_lon, io.site_lat, n_sector, sector0_deg, n_bin, thresholds, io.counts, d_max,
                            ctx->stream))
        return -1;
    if (scan_download_planes(ctx, io, n_sector, site_dir_max, d_max)) return -1;
    return scan_download(ctx, io, counts, nullptr);
}

int tcr_directional_pairs(tcr_ctx *ctx, int64_t *pairs) { return ctx ? scan_pairs(ctx, ctx->an.dr, "tcr_directional", pairs) : -1; }

}  // extern "C"
