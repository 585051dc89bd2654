// Closest approach behind the C ABI (include/tcrisk_hip.h, "closest approach" section): how every storm passed every site.  The
// record of a storm nearest to the site (the closest point of approach, CPA), what the storm was doing there, and how many storms
// of every group passed within each of up to eight distance bands at or above each of a list of intensities, from one scan.
//
//   CPA(site, storm)         = the record of least haversine argument q among those with q <= a_R; the earliest on equal q
//   planes[k][site][storm]   = distance_km, time_h, v, speed, heading_deg, side_km, rmax_km of that record (NaN: none included)
//   counts[site][group][band][bin] = #storms of the group with distance_km <= band_km[band] and v >= thr[bin]
//
// A user of the site scan (tcr_sitescan.h: tiling, culling, the mode protocol).  What is the approach's own:
//   CaRec             the record (128 bytes): the five half-angle terms and idx, the record's index in its track, then the
//                     full-angle terms of the centre and the payload of a winner: v, the motion (ue, un) of the record's segment,
//                     rm, its speed and heading.  uniform() loads what add reads, the five terms and idx: 48 bytes of the
//                     record's first 64-byte line.  With idx behind rm, in the record's second line, the record loop fetched
//                     two lines per record through the scalar cache and the scan took 186 ms where it now takes 133
//                     (profiles/approach_bench.txt);
//   k_approach_prep   one wave per storm: finds the track (ballot), stages (lon, lat, v, rm) of every sample, then writes one record
//                     per sample and sub-sample, positions as wf_sub_record's.  All trigonometry, the square root of the speed,
//                     the atan2 of the heading and the Willoughby exp are here;
//   ScanClosest<NB>   the mode (NB = 4 or 8 band accumulators), the engine's argmin with a payload.  A lane keeps { q, idx } of a
//                     storm: add is one strict compare and two selects on scalar-loaded values, no payload arithmetic and no
//                     record slot beyond idx.  end_storm is the only vector read of records: a lane with a winner gathers
//                     row[idx] with an ordinary per-lane load, forms the seven values, writes the planes the call asked for
//                     (their pointers travel in the policy: the rows of the stacked histogram are the bands, which have no
//                     planes of their own) and hands every band to ScanStack::finish with `distance <= band` as its `any`;
//   ApproachScan<NB>  the policy: the rows, the planes, the bands, the units.
//
// The CPA is taken on the records: the minimum along the chord between two records is not modelled, substeps is the refinement.
//
// Bit-identity, by the engine's argument for an order-dependent mode (tcr_sitescan.h): one lane owns a (site, storm); its records
// arrive segment-ascending and record-ascending inside a segment; culling is conservative, so a culled storm or segment holds no
// included record, and padding records fail q <= a_R.  The strict `<` keeps the earliest record of the least q, and that least q
// and its first index are functions of the storm's included records alone.  So the argmin and its tie rule do not depend on the
// launch shape, the site order, the storm order or the chunking; every plane is a function of the winner and the site, the band
// test is made on the very double written to plane 0, and the counts are integers.

namespace {

constexpr int kCaPlanes = 7;
constexpr double kCaMaxBandKm = 5000.0;

struct CaStage { double lon, lat, v, rm; };              // one track sample (32 bytes)

struct CaRec {
    double sp, cp, sl, cl, cosp;
    int64_t idx;                            // right behind the five terms: what the record loop reads is one 64-byte line
    double sinp, sinl, cosl, v, ue, un, rm, speed, heading, pad0;
    static __device__ __forceinline__ CaRec uniform(const CaRec *p)
    {
        const double *d = &p->sp;
        return CaRec{hz_uniform(d), hz_uniform(d + 1), hz_uniform(d + 2), hz_uniform(d + 3), hz_uniform(d + 4), hz_uniform(&p->idx),
                     0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    }
    __device__ void centre(HzCap *out) const { out->x = cosp * cosl; out->y = cosp * sinl; out->z = sinp; }
};
static_assert(sizeof(CaRec) == 128, "CaRec is 16 slots of 8 bytes");

struct CaPrepArgs {
    const double *lon, *lat, *vmax, *rmax;  // rmax: [n_trk][stride] km, or NULL
    int64_t n_trk, n_t, stride;
    double dt, rm_const;                    // rm_const > 0: rm everywhere (km); 0: Willoughby et al. (2006)
    int32_t sub;
    CaStage *stage;                         // [n_trk][n_t]
    ScanRows<CaRec> out;
};

// record q of a staged track of n >= 2 samples: sample q / sub, or the sub-sample at tau = (q % sub) / sub after it, with the
// motion of the segment it lies on (the track's last record: the last segment's)
__device__ __forceinline__ CaRec ca_record(const CaStage *st, int q, int sub, int64_t n, double dt)
{
    const int k = q / sub, j = q - k * sub;
    const CaStage p = st[k];
    double x = p.lon, y = p.lat, v = p.v, rm = p.rm;
    if (j != 0) {
        const CaStage p1 = st[k + 1];
        const double tau = (double)j / (double)sub;
        double dl = p1.lon - p.lon;
        dl -= 360.0 * floor((dl + 180.0) / 360.0);      // [-180, 180)
        x = p.lon + tau * dl; y = p.lat + tau * (p1.lat - p.lat); v = p.v + tau * (p1.v - p.v); rm = p.rm + tau * (p1.rm - p.rm);
    }
    const int64_t ks = k < n - 1 ? k : n - 2;
    const CaStage a = st[ks], b = st[ks + 1];
    double dl = b.lon - a.lon;
    dl -= 360.0 * floor((dl + 180.0) / 360.0);
    const double phim = (a.lat + b.lat) / 2.0;
    CaRec r;
    const double hp = y * (kPi / 360.0), hl = x * (kPi / 360.0), phi = y * (kPi / 180.0), lam = x * (kPi / 180.0);
    r.sp = sin(hp); r.cp = cos(hp); r.sl = sin(hl); r.cl = cos(hl);
    r.cosp = cos(phi); r.sinp = sin(phi); r.sinl = sin(lam); r.cosl = cos(lam);
    r.v = v; r.rm = rm;
    r.ue = kWfEarthR * cos(phim * (kPi / 180.0)) * (dl * (kPi / 180.0)) / dt;
    r.un = kWfEarthR * ((b.lat - a.lat) * (kPi / 180.0)) / dt;
    r.idx = q;
    r.speed = sqrt(r.ue * r.ue + r.un * r.un);
    double h = NAN;
    if (r.ue != 0.0 || r.un != 0.0) {
        h = atan2(r.ue, r.un) * (180.0 / kPi);
        if (h < 0.0) h += 360.0;
        if (h >= 360.0) h = 0.0;                        // (-tiny + 360 rounds to 360)
    }
    r.heading = h; r.pad0 = 0.0;
    return r;
}

__global__ __launch_bounds__(64) void k_approach_prep(CaPrepArgs a)
{
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t o = s * a.stride;
    const double *lon = a.lon + o, *lat = a.lat + o, *vv = a.vmax + o;
    // the track: the samples before the first one with a non-finite input
    const int64_t n = scan_track_len(a.n_t, [&](int64_t j) { return !(isfinite(lon[j]) && isfinite(lat[j]) && isfinite(vv[j])); });
    CaStage *st = a.stage + s * a.n_t;
    CaRec *row = a.out.rec + s * a.out.n_seg_max * kHzSeg;
    bool bad_rm = false;
    if (n >= 2)
        for (int64_t k = lane; k < n; k += 64) {
            const double y = lat[k], v = vv[k];
            const double rm = a.rmax ? a.rmax[o + k] : (a.rm_const > 0.0 ? a.rm_const : 46.4 * exp(-0.0155 * v + 0.0169 * fabs(y)));
            if (!(isfinite(rm) && rm > 0.0)) bad_rm = true;
            st[k] = CaStage{lon[k], y, v, rm};
        }
    const bool drop = __ballot(bad_rm) != 0;
    const int nr = (n >= 2 && !drop) ? (int)((n - 1) * a.sub + 1) : 0;
    __syncthreads();                                    // the records read stage entries other lanes wrote
    for (int q = lane; q < nr; q += 64) row[q] = ca_record(st, q, a.sub, n, a.dt);
    scan_finish_row(a.out, s, nr);
}

// the mode of ApproachScan (header comment), on ScanStack with the bands for rows
template <int NB>
struct ScanClosest {
    struct Storm {
        double q = INFINITY;                // the least haversine argument so far,
        int64_t idx = -1;                   // and the first record that has it (-1: none included)
    };
    double sinp, cosp, sinl, cosl;          // the lane's site: the full-angle terms of ScanSite, for the side of the track
    template <class P> __device__ __forceinline__ void begin(const P &pol, const ScanLane &c)
    {
        ScanStack::begin(c, pol.out.n_row, pol.out.n_hbin);
        const double phi = c.a.site_lat[c.my] * (kPi / 180.0), lam = c.a.site_lon[c.my] * (kPi / 180.0);
        sinp = sin(phi); cosp = cos(phi); sinl = sin(lam); cosl = cos(lam);
    }
    template <class P, class Rec> __device__ __forceinline__ void add(const P &, Storm &st, const ScanSite &, const Rec &p, double q)
    {
        const bool closer = q < st.q;       // strict: on equal q the earlier record stays
        st.q = closer ? q : st.q;
        st.idx = closer ? p.idx : st.idx;
    }
    template <class P> __device__ __forceinline__ void end_storm(const P &pol, const ScanLane &c, const Storm &st, int64_t s, bool)
    {
        const bool any = st.idx >= 0;
        double val[kCaPlanes];
#pragma unroll
        for (int k = 0; k < kCaPlanes; ++k) val[k] = NAN;
        if (any) {
            const CaRec *w = pol.rec + s * pol.row_len + st.idx;       // the winner: a per-lane load
            const double d = (kWfEarthR / 1000.0) * scan_pair_angle(st.q);
            const double ue = w->ue, un = w->un;
            // (e, nn): the centre -> site direction, WindScan::at_angle's expressions
            const double sdl = sinl * w->cosl - cosl * w->sinl, cdl = cosl * w->cosl + sinl * w->sinl;
            const double e = cosp * sdl, nn = w->cosp * sinp - w->sinp * (cosp * cdl);
            const double cross = ue * nn - un * e;
            val[0] = d;
            val[1] = (double)st.idx * pol.unit;
            val[2] = w->v;
            val[3] = w->speed;
            val[4] = w->heading;
            val[5] = cross < 0.0 ? d : (cross > 0.0 ? -d : 0.0);
            val[6] = w->rm;
        }
        if (c.valid) {
#pragma unroll
            for (int k = 0; k < kCaPlanes; ++k)
                if (pol.plane[k]) pol.plane[k][c.site * c.a.n_trk + s] = val[k];        // (wave-uniform)
        }
#pragma unroll
        for (int r = 0; r < NB; ++r)
            if (r < pol.out.n_row) ScanStack::finish(pol.out, c, r, s, any && val[0] <= pol.band[r], val[2]);    // (wave-uniform)
    }
    template <class P> __device__ __forceinline__ void end_chunk(const P &pol, const ScanLane &c) { ScanStack::end_chunk(c, pol.out.n_row, pol.out.n_hbin); }
};

// the policy of k_site_scan<ApproachScan<NB>>: NB band accumulators (the call's n_band <= NB)
template <int NB>
struct ApproachScan {
    using Rec = CaRec;
    using Mode = ScanClosest<NB>;
    static constexpr int kUnroll = 4;
    const CaRec *rec;                       // the rows of the call, for the gather of a winner
    int64_t row_len;                        // records of a row: n_seg_max * kHzSeg
    double band[NB];                        // km, ascending; -inf past n_band
    double unit;                            // hours per record index: dt_s / (3600 substeps)
    double *plane[kCaPlanes];               // [n_site][n_trk] each, or NULL
    ScanStackOut<NB> out;                   // n_band rows; no planes of their own (all NULL)
};

int approach_check(tcr_ctx *ctx, const tcr_hazard_tracks *t, const tcr_approach_params *p, int64_t n_site, const double *site_lon,
                   const double *site_lat, int32_t n_band, const double *band_km, int32_t n_bin, const double *thr, const int32_t *counts,
                   const double *rmax_km)
{
    if (!t || !p || !site_lon || !site_lat || !band_km || !thr || !counts || !t->lon || !t->lat || !t->vmax || !t->group_off)
        return fail(ctx, "tcr_approach: NULL argument");
    if (!(p->dt_s > 0.0 && std::isfinite(p->dt_s))) return fail(ctx, "tcr_approach: dt_s must be finite and > 0");
    if (p->substeps < 1 || p->substeps > kWfMaxSub) return fail(ctx, "tcr_approach: substeps must be in [1, 64]");
    if (!(p->rmax_const_km >= 0.0 && std::isfinite(p->rmax_const_km)) || (rmax_km && p->rmax_const_km != 0.0))
        return fail(ctx, "tcr_approach: rmax_const_km must be finite and >= 0, and 0 when the rmax_km plane is given");
    if (scan_check(ctx, "tcr_approach", t, 1 << 20, "1 <= n_t <= 2^20", n_site, n_bin, thr)) return -1;
    if (scan_stack_check(ctx, "tcr_approach", "band", n_band, n_bin)) return -1;
    for (int r = 0; r < n_band; ++r)
        if (!std::isfinite(band_km[r]) || !(band_km[r] > 0.0) || band_km[r] > kCaMaxBandKm || (r > 0 && !(band_km[r] > band_km[r - 1])))
            return fail(ctx, "tcr_approach: band_km must be finite, > 0, strictly ascending and at most 5000");
    return 0;
}

struct CaCall {
    const tcr_hazard_tracks *t;
    const double *rmax_km;
    const tcr_approach_params *prm;
    int32_t n_band, n_bin;
    const double *band_km;
    double *const *planes;
};

template <int NB>
hipError_t approach_launch(const CaCall &d, const ScanRows<CaRec> &rows, const ScanLaunch &L, void *stage)
{
    ApproachScan<NB> pol{};
    pol.rec = rows.rec; pol.row_len = rows.n_seg_max * kHzSeg;
    for (int r = 0; r < NB; ++r) {
        pol.band[r] = r < d.n_band ? d.band_km[r] : -INFINITY;
        pol.out.plane[r] = nullptr;
    }
    pol.unit = d.prm->dt_s / (3600.0 * d.prm->substeps);
    for (int k = 0; k < kCaPlanes; ++k) pol.plane[k] = d.planes ? d.planes[k] : nullptr;
    pol.out.n_row = d.n_band; pol.out.n_hbin = d.n_bin;
    const CaPrepArgs p{d.t->lon, d.t->lat, d.t->vmax, d.rmax_km, d.t->n_trk, d.t->n_t, d.t->row_stride, d.prm->dt_s,
                       d.prm->rmax_const_km, d.prm->substeps, static_cast<CaStage *>(stage), rows};
    return scan_launch(k_approach_prep, p, rows, L, pol);
}

}  // namespace

extern "C" {

int tcr_approach_dev(tcr_ctx *ctx, const tcr_hazard_tracks *t, const double *rmax_km, const tcr_approach_params *prm, int64_t n_site,
                     const double *site_lon, const double *site_lat, int32_t n_band, const double *band_km, int32_t n_bin,
                     const double *thresholds, int32_t *counts, double *const *planes, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || approach_check(ctx, t, prm, n_site, site_lon, site_lat, n_band, band_km, n_bin, thresholds, counts, rmax_km)) return -1;
    const int64_t n_rec = (t->n_t - 1) * prm->substeps + 1;
    const size_t n_stage = (size_t)std::max<int64_t>(1, t->n_trk * t->n_t);
    const CaCall d{t, rmax_km, prm, n_band, n_bin, band_km, planes};
    // (the modes of every NB have the one shape)
    return scan_run<CaRec>(ctx, ctx->an.ca, "tcr_approach", t, scan_plan(t, n_site, kScanAnyChunk),
                           ScanStack::shape(n_band, n_bin, 0, thresholds), n_rec, n_stage * sizeof(CaStage), n_site, site_lon, site_lat,
                           band_km[n_band - 1], kWfEarthR / 1000.0, counts, nullptr, st,
                           [&](const ScanRows<CaRec> &rows, const ScanLaunch &L, void *stage) {
        return n_band <= 4 ? approach_launch<4>(d, rows, L, stage) : approach_launch<kScanMaxRow>(d, rows, L, stage);
    });
}

int tcr_approach_host(tcr_ctx *ctx, const tcr_hazard_tracks *t, const double *rmax_km, const tcr_approach_params *prm, int64_t n_site,
                      const double *site_lon, const double *site_lat, int32_t n_band, const double *band_km, int32_t n_bin,
                      const double *thresholds, int32_t *counts, double *const *planes)
{
    if (!enter(ctx) || approach_check(ctx, t, prm, n_site, site_lon, site_lat, n_band, band_km, n_bin, thresholds, counts, rmax_km)) return -1;
    DevBuf B;
    tcr_hazard_tracks d;
    const ScanHostIO io = scan_host_io(B, t, n_site, site_lon, site_lat, n_band * n_bin, false);
    const double *d_rmax = nullptr;
    if (rmax_km) d_rmax = t->n_trk > 0 ? B.put(rmax_km, (size_t)t->n_trk * t->row_stride) : B.get<double>(1);
    double *d_planes[kCaPlanes] = {};
    if (!hazard_tracks_upload(B, t, &d) || !io.ok || (rmax_km && !d_rmax) || !scan_host_planes(B, io, kCaPlanes, planes, d_planes))
        return fail(ctx, "tcr_approach_host: device allocation / upload failed");
    if (tcr_approach_dev(ctx, &d, d_rmax, prm, n_site, io.site_lon, io.site_lat, n_band, band_km, n_bin, thresholds, io.counts, d_planes,
                         ctx->stream))
        return -1;
    if (scan_download_planes(ctx, io, kCaPlanes, planes, d_planes)) return -1;
    return scan_download(ctx, io, counts, nullptr);
}

int tcr_approach_pairs(tcr_ctx *ctx, int64_t *pairs) { return ctx ? scan_pairs(ctx, ctx->an.ca, "tcr_approach", pairs) : -1; }

}  // extern "C"
