// Rain accumulation windows behind the C ABI (include/tcrisk_hip.h, "rain accumulation windows" section): the largest rain depth
// every storm leaves at every site within any m consecutive sample intervals, for up to eight window lengths m at once, and how
// many storms of every group reach each of a list of depths, from one scan of the ensemble.  Between the rainfall footprint's
// two statistics: the peak rate is the window of no length, the storm total the window longer than the track.
//
//   h = dt_s / (3600 substeps) hours;  rho_q = the rate of record q at the site if the pair is included, else 0
//   I_q = (h / 2) (rho_q + rho_q+1),  q = 0 .. nr - 2               the trapezoid of one sub-interval
//   T_k = sum of I_q over q < k substeps, in ascending q,  T_0 = 0   the depth up to sample k = 0 .. n - 1
//   A_i = max over k of T_k - T_max(k - m_i, 0)                      (mm; NaN when no record of the storm is included)
//   site_window[i][site][storm] = A_i;   counts[site][group][i][b] = #storms of the group with A_i >= thresholds[b]
//
// A user of the site scan (tcr_sitescan.h: tiling, culling, the mode protocol) on the rainfall footprint's records: the prep
// kernel is k_rain_prep itself, the rate of a pair is RainScan<false>'s.  What is the accumulation's own:
//   AccumScan<NW>     the policy of k_site_scan: the rate, the half step h / 2, the windows and where the planes go.  The record's
//                     index in its track and whether it is the track's last are RfRec's q and end;
//   ScanWindows<NW>   the mode (1 <= NW <= kScanMaxRow): the first whose state of a storm is a time series.  Per lane and storm
//                     in registers: the index and rate of the last included record, the running T up to that record, the number of
//                     sample boundaries passed, the first boundary this storm wrote, the ring position and best[NW] (fixed arrays,
//                     fully unrolled, never indexed by a run-time value).  Per lane in the wave's LDS, behind the histogram
//                     cells: a ring of m_max + 1 values of T at the last sample boundaries, [slot][lane] in doubles, so that a
//                     lane stays in its own pair of banks whatever slot it is at (the lanes' catch-up loops are at different
//                     slots).  Per storm each of the call's n_row windows has the value best[i] (NaN when no record was
//                     included): a row of the stacked histogram (ScanStack, tcr_sitescan.h: the plane, the rank, the partial
//                     counts).
//
// k_site_scan calls add only for included pairs and skips culled segments for the whole wave, so the mode catches up inside add
// and end_storm.  The records between the last included one and this one had rate 0: T first takes (h / 2) rho_last, is constant
// over the gap, and then takes (h / 2) rho_q; for neighbouring records it takes (h / 2)(rho_last + rho_q).  Every sample boundary
// passed is written to the ring and evaluated against all windows; a boundary before the storm's first written one has T = 0 and
// is never read, so the ring is not cleared per storm.  A gap of more than m_max + 1 boundaries evaluates its first one (T is
// constant over the gap and T_k-m does not decrease with k, so no later one of the gap can win), fills the ring with the constant
// and jumps.  end_storm adds the trailing half interval when the last included record is not the track's last, and evaluates the
// next boundary (no later one can win, as before).
//
// Bit-identity: tcr_sitescan.h's argument for a per-lane sum in record order carries over.  The definition's T is a sequential
// sum whose terms for excluded records are exact zeros: (h / 2)(rho + 0) is (h / 2) rho bit for bit, and adding 0.0 changes no
// bits of a T >= 0.  So the lazy T is the definition's T whatever was culled, skipped or excluded: one lane, one accumulator, the
// included records in record order.  The ring holds this lane's own T of this storm only, T - T' and max are functions of their
// operands, and nothing reduces a value across lanes or chunks; the counts are integers.  So every output is the same bits
// whatever the launch shape, the site order and the storm order.  A is non-decreasing in m exactly: T is a non-decreasing
// sequence (its terms are >= 0) and fp64 subtraction is monotone in each operand.

namespace {

constexpr int kAcMaxSamples = 96;           // the longest window, in samples
constexpr size_t kAcMaxLds = 65536;         // of a wave: what a launch may ask for without an attribute

// the mode of AccumScan (header comment), on ScanStack with the windows for rows; in the wave's LDS behind the histogram's cells
// the ring, [n_slot][64] of double
template <int NW>
struct ScanWindows {
    struct Storm {
        int32_t last = -1;                  // the last included record (-1: none yet),
        int32_t end = 0;                    // whether it is the track's last,
        double rho = 0.0;                   // and its rate
        double T = 0.0;                     // the depth up to record `last`
        int32_t nb = 0;                     // boundaries 0 .. nb - 1 are behind `last`: evaluated, or T = 0 before the first one written
        int32_t k0 = 0;                     // the first boundary written: T_k = 0 for k < k0
        int32_t slot = 0;                   // where boundary nb goes in the ring
        double best[NW] = {};
    };
    double *ring;                           // this lane's column of the ring: slot j is ring[j * 64]
    int32_t n_slot;                         // m_max + 1
    static ScanShape shape(int32_t n_window, int32_t n_hbin, int32_t m_max, const double *thr)
    {
        return ScanStack::shape(n_window, n_hbin, sizeof(double) * 64 * ((size_t)m_max + 1), thr);
    }
    template <class P> __device__ __forceinline__ void begin(const P &pol, const ScanLane &c)
    {
        ScanStack::begin(c, pol.out.n_row, pol.out.n_hbin);
        ring = reinterpret_cast<double *>(c.lds + pol.out.n_row * (pol.out.n_hbin + 1) * 64) + c.lane;
        n_slot = pol.n_slot;
    }
    // boundary st.nb, which has (or would have) the ring position st.slot, has the depth T: every window's T - T_(nb - m), where
    // a boundary before k0 (and so any before 0) is 0.  m >= 1: st.slot itself is never read
    template <class P> __device__ __forceinline__ void eval(const P &pol, Storm &st, double T) const
    {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            if (i < pol.out.n_row) {                    // (wave-uniform)
                int s = st.slot - pol.m[i];
                if (s < 0) s += n_slot;                 // (m <= m_max = n_slot - 1: 0 <= s < n_slot)
                const double prev = st.nb - pol.m[i] < st.k0 ? 0.0 : ring[s * 64];
                st.best[i] = fmax(st.best[i], T - prev);
            }
        }
    }
    template <class P> __device__ __forceinline__ void emit(const P &pol, Storm &st, double T) const
    {
        ring[st.slot * 64] = T;
        eval(pol, st, T);
        st.slot = st.slot + 1 == n_slot ? 0 : st.slot + 1;
        ++st.nb;
    }
    template <class P, class Rec> __device__ __forceinline__ void add(const P &pol, Storm &st, const ScanSite &me, const Rec &p, double q)
    {
        const double rho = pol.value(me, p, q);
        const int32_t iq = (int32_t)p.q, kq = iq / pol.substeps;       // (wave-uniform)
        const bool on = kq * pol.substeps == iq;                        // the record is sample kq: boundary kq ends here
        if (st.last >= 0 && iq == st.last + 1) st.T += pol.hh * (st.rho + rho);
        else {
            const int32_t kend = on ? kq - 1 : kq;                      // the last boundary before this record
            if (st.last < 0) {                                          // nothing before: T_k = 0 up to kend
                st.nb = st.k0 = kend + 1;
                if (iq > 0) st.T = pol.hh * rho;
            } else {
                st.T += pol.hh * st.rho;                                // the half interval behind the last record; then a constant
                const int32_t n = kend - st.nb + 1;
                if (n > n_slot) {
                    eval(pol, st, st.T);
                    for (int j = 0; j < n_slot; ++j) ring[j * 64] = st.T;
                    st.nb = kend + 1;                                   // (every slot holds the constant: any position will do)
                } else
                    for (int j = 0; j < n; ++j) emit(pol, st, st.T);
                st.T += pol.hh * rho;                                   // the half interval before this record
            }
        }
        if (on) emit(pol, st, st.T);
        st.last = iq; st.rho = rho; st.end = (int32_t)p.end;
    }
    // the trailing half interval, and a row per window; a storm without an included record counts nowhere
    template <class P> __device__ __forceinline__ void end_storm(const P &pol, const ScanLane &c, const Storm &st0, int64_t s, bool)
    {
        Storm st = st0;
        const bool any = st.last >= 0;
        if (any && !st.end) eval(pol, st, st.T + pol.hh * st.rho);
#pragma unroll
        for (int i = 0; i < NW; ++i)
            if (i < pol.out.n_row) ScanStack::finish(pol.out, c, i, s, any, any ? st.best[i] : NAN);        // (wave-uniform)
    }
    template <class P> __device__ __forceinline__ void end_chunk(const P &pol, const ScanLane &c) { ScanStack::end_chunk(c, pol.out.n_row, pol.out.n_hbin); }
};

// the policy of k_site_scan<AccumScan<NW>>: NW accumulators (the call's n_window <= NW)
template <int NW>
struct AccumScan {
    using Rec = RfRec;
    using Mode = ScanWindows<NW>;
    static constexpr int kUnroll = 2;       // (1 and 4 measured within 3 % of it: profiles/accumulation_unroll_ab.txt)
    RainScan<false> rain;
    double hh;                              // h / 2: hours per half sub-step
    int32_t substeps, n_slot;
    int32_t m[NW];                          // window lengths in samples, ascending; 0 past n_window (T_k - T_k: never wins)
    ScanStackOut<NW> out;                   // n_window rows; the planes are site_window[i]
    __device__ __forceinline__ double value(const ScanSite &s, const RfRec &p, double q) const { return rain.value(s, p, q); }
};

int accumulation_check(tcr_ctx *ctx, const tcr_hazard_tracks *t, const tcr_rain_params *p, int64_t n_site, const double *site_lon,
                       const double *site_lat, int32_t n_window, const int32_t *window_samples, int32_t n_bin, const double *thr,
                       const int32_t *counts)
{
    if (!window_samples) return fail(ctx, "tcr_accumulation: NULL argument");
    if (rainfall_check(ctx, t, p, n_site, site_lon, site_lat, n_bin, thr, counts, "tcr_accumulation")) return -1;
    if (p->stat != TCR_RAIN_TOTAL) return fail(ctx, "tcr_accumulation: stat must be TCR_RAIN_TOTAL (0)");
    if (scan_stack_check(ctx, "tcr_accumulation", "window", n_window, n_bin)) return -1;
    for (int i = 0; i < n_window; ++i)
        if (window_samples[i] < 1 || window_samples[i] > kAcMaxSamples || (i > 0 && window_samples[i] <= window_samples[i - 1]))
            return fail(ctx, "tcr_accumulation: window_samples must be in [1, 96] and strictly ascending");
    if (ScanWindows<kScanMaxRow>::shape(n_window, n_bin, window_samples[n_window - 1], thr).lds > kAcMaxLds)
        return fail(ctx, "tcr_accumulation: 512 (longest window + 1) + 256 n_window (n_bin + 1) must be <= 65536 (the LDS of a wave)");
    return 0;
}

struct AcCall {
    const tcr_hazard_tracks *t;
    const tcr_rain_params *prm;
    int32_t n_window, n_bin;
    const int32_t *m;
    double *const *site_window;
};

template <int NW>
hipError_t accumulation_launch(const AcCall &d, const ScanRows<RfRec> &rows, const ScanLaunch &L)
{
    AccumScan<NW> pol{};
    pol.hh = 0.5 * (d.prm->dt_s / (3600.0 * d.prm->substeps));
    pol.substeps = d.prm->substeps; pol.out.n_row = d.n_window; pol.out.n_hbin = d.n_bin;
    pol.n_slot = d.m[d.n_window - 1] + 1;
    for (int i = 0; i < NW; ++i) {
        pol.m[i] = i < d.n_window ? d.m[i] : 0;
        pol.out.plane[i] = (d.site_window && i < d.n_window) ? d.site_window[i] : nullptr;
    }
    return scan_launch(k_rain_prep, rain_prep_args(d.t, d.prm, rows), rows, L, pol);
}

}  // namespace

extern "C" {

int tcr_accumulation_dev(tcr_ctx *ctx, const tcr_hazard_tracks *t, const tcr_rain_params *prm, int64_t n_site, const double *site_lon,
                         const double *site_lat, int32_t n_window, const int32_t *window_samples, int32_t n_bin, const double *thresholds,
                         int32_t *counts, double *const *site_window, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || accumulation_check(ctx, t, prm, n_site, site_lon, site_lat, n_window, window_samples, n_bin, thresholds, counts)) return -1;
    const int64_t n_rec = (t->n_t - 1) * prm->substeps + 1;
    const AcCall d{t, prm, n_window, n_bin, window_samples, site_window};
    // (the modes of every NW have the one shape)
    return scan_run<RfRec>(ctx, ctx->an.ac, "tcr_accumulation", t, scan_plan(t, n_site, kScanAnyChunk),
                           ScanWindows<kScanMaxRow>::shape(n_window, n_bin, window_samples[n_window - 1], thresholds), n_rec, 0, n_site,
                           site_lon, site_lat, prm->r_out_km, kWfEarthR / 1000.0, counts, nullptr, st,
                           [&](const ScanRows<RfRec> &rows, const ScanLaunch &L, void *) {
        return n_window <= 4 ? accumulation_launch<4>(d, rows, L) : accumulation_launch<kScanMaxRow>(d, rows, L);
    });
}

int tcr_accumulation_host(tcr_ctx *ctx, const tcr_hazard_tracks *t, const tcr_rain_params *prm, int64_t n_site, const double *site_lon,
                          const double *site_lat, int32_t n_window, const int32_t *window_samples, int32_t n_bin, const double *thresholds,
                          int32_t *counts, double *const *site_window)
{
    if (!enter(ctx) || accumulation_check(ctx, t, prm, n_site, site_lon, site_lat, n_window, window_samples, n_bin, thresholds, counts))
        return -1;
    DevBuf B;
    tcr_hazard_tracks d;
    const ScanHostIO io = scan_host_io(B, t, n_site, site_lon, site_lat, n_window * n_bin, false);
    double *d_win[kScanMaxRow] = {};
    if (!hazard_tracks_upload(B, t, &d) || !io.ok || !scan_host_planes(B, io, n_window, site_window, d_win))
        return fail(ctx, "tcr_accumulation_host: device allocation / upload failed");
    if (tcr_accumulation_dev(ctx, &d, prm, n_site, io.site_lon, io.site_lat, n_window, window_samples, n_bin, thresholds, io.counts, d_win,
                             ctx->stream))
        return -1;
    if (scan_download_planes(ctx, io, n_window, site_window, d_win)) return -1;
    return scan_download(ctx, io, counts, nullptr);
}

int tcr_accumulation_pairs(tcr_ctx *ctx, int64_t *pairs) { return ctx ? scan_pairs(ctx, ctx->an.ac, "tcr_accumulation", pairs) : -1; }

}  // extern "C"
