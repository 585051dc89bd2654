// Wind footprint behind the C ABI (include/tcrisk_hip.h, "wind footprint" section): the peak wind every storm produces at every
// site, from the Emanuel & Rotunno (2011, eq. 36) radial profile around the centre plus the asymmetry of axi_to_max_wind
// (wind/tc_wind.py), so that at r = rm on the azimuth of maximum wind it is the pipeline's vmax_trks.
//
//   site_max[site][storm] = max over the samples and sub-samples with haversine(site, centre) <= r_out of |V(r) t + (V / v) A|
//   counts[site][group][bin] = #storms of the group with site_max >= thr[bin]
//
// Two kernels of this file and the hazard's reduction:
//   k_wind_prep      one wave per storm: finds the track (ballot), stages (lon, lat, v, rm, A) of every track sample with the
//                    translation speed in the operation order of vmax_at (tcr_kernels.hip), then writes one record per sample and
//                    sub-sample with every wave-uniform term a pair needs, and the hazard's bounding caps (tcr_hazard.hip) of the
//                    storm and of every kHzSeg-record segment;
//   k_wind_main      one wave per (tile of 64 sites, chunk of storms of one group), as k_hazard_main: every lane holds one site's
//                    terms in registers, the records come through scalar loads, storms and segments whose cap is farther than r_out
//                    from the tile's cap are skipped.  The haversine argument a is tested against a_out first (no trigonometry);
//                    only included lanes pay for asin, the square roots and the profile;
//   k_hazard_reduce  sums the integer per-chunk partial counts of each group.
//
// Per included pair (c: centre, s: site; the record holds the centre's terms):
//   r = 2 R asin(sqrt(a))
//   V = r (2 Mm / (rm^2 + r^2) - f/2)            c = 1: ratio = 2 x^2 / (1 + x^2), no pow (the launch-uniform template branch)
//   V = (Mm ratio - (f/2) r^2) / r, V(0) = 0     otherwise
//   |w| = V |t + A / v| = V sqrt(1 + |A / v|^2 + d_e b_n - d_n b_e),  b = 2 h A / v
// with sin and cos of (lam_s - lam_c) from the difference identity of the full-angle terms.  |A| = min(|U|, v / 2), so the root's
// argument is >= 1/4.  A sample with v <= 0 carries Mm = f/2 = 0 and b = 0: its wind is 0 wherever it is included.
//
// Culling is the hazard's (caps padded by kHzPad, test margin kHzDotPad), so a skipped pair is always farther than r_out.  A pair's
// value does not depend on which other pairs are evaluated, and max and integer sums do not depend on order: the results are
// bit-identical whatever the launch shape, the site order and the storm order.

namespace {

constexpr int kWfMaxSub = 64;
constexpr double kWfEarthR = 6.3781 * 1e6;          // util/constants.py earth_R (m): the pipeline's P.earth_R
constexpr double kWfOmega = 7.292e-5;               // s^-1

struct WfStage { double lon, lat, v, rm, ae, an, pad0, pad1; };      // one track sample (64 bytes)
// one sample or sub-sample (128 bytes): half-angle terms of the centre (distance), full-angle terms (direction), rm (m), Mm, f / 2,
// 1 + |A / v|^2 and b = 2 h A / v
struct WfRec { double sp, cp, sl, cl, cosp, sinp, sinl, cosl, rm, mm, f2, a2, be, bn, pad0, pad1; };

struct WfPrepArgs {
    const double *lon, *lat, *v, *u250, *v250, *u850, *v850, *rmax;   // rmax: [n_trk][stride] km, or NULL
    int64_t n_trk, n_t, stride;
    double dt, rm_const;                    // rm_const > 0: rm everywhere (km); 0: Willoughby et al. (2006)
    int32_t sub;
    WfStage *stage;                         // [n_trk][n_t]
    WfRec *rec;                             // [n_trk][n_seg_max * kHzSeg]
    HzCap *seg;                             // [n_trk][n_seg_max]
    HzCap *storm;                           // [n_trk]
    int32_t *cnt;                           // [n_trk] records
    int64_t n_seg_max;
};

struct WfMainArgs {
    const WfRec *rec;
    const HzCap *seg, *storm;
    const int32_t *cnt;
    const int64_t *chunks;                  // [n_chunk][3]: storm begin, storm end, group
    const double *site_lon, *site_lat;
    int64_t n_site, n_tile, n_seg_max, n_trk;
    double a_out, r_ang;                    // a threshold of r_out, r_out in radians
    double c, two_c, inv_exp;               // profile: c, 2 - c, 1 / (2 - c)
    int32_t n_bin;
    double thr[kHzMaxBin];
    int32_t *part;                          // [n_chunk][n_site][n_bin]
    double *site_max;                       // [n_site][n_trk] or NULL
    unsigned long long *pairs;              // pairs evaluated (after culling)
};

__device__ __forceinline__ WfRec wf_uniform(const WfRec *p)
{
    const double *d = &p->sp;
    return WfRec{hz_uniform(d), hz_uniform(d + 1), hz_uniform(d + 2), hz_uniform(d + 3), hz_uniform(d + 4), hz_uniform(d + 5),
                 hz_uniform(d + 6), hz_uniform(d + 7), hz_uniform(d + 8), hz_uniform(d + 9), hz_uniform(d + 10), hz_uniform(d + 11),
                 hz_uniform(d + 12), hz_uniform(d + 13), 0.0, 0.0};
}

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
    r.pad0 = r.pad1 = 0.0;
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

// hz_cap over records: centre = the record at `mid`, radius = the largest angle from it
__device__ void wf_cap(const WfRec *row, int b, int e, HzCap *out)
{
    const int lane = threadIdx.x;
    const WfRec &c = row[b + (e - b) / 2];
    double r = 0.0;
    for (int j = b + lane; j < e; j += 64) {
        const WfRec &p = row[j];
        r = fmax(r, hz_angle(hz_a(c.sp, c.cp, c.sl, c.cl, c.cosp, p.sp, p.cp, p.sl, p.cl, p.cosp)));
    }
    r = wave_max(r) + kHzPad;
    if (lane == 0) {
        out->x = c.cosp * c.cosl; out->y = c.cosp * c.sinl; out->z = c.sinp;
        out->cr = cos(r); out->sr = sin(r); out->r = r; out->pad0 = out->pad1 = 0.0;
    }
}

__global__ __launch_bounds__(64) void k_wind_prep(WfPrepArgs a)
{
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t o = s * a.stride;
    const double *lon = a.lon + o, *lat = a.lat + o, *vv = a.v + o;
    const double *u2 = a.u250 + o, *v2 = a.v250 + o, *u8 = a.u850 + o, *v8 = a.v850 + o;
    // the track: the samples before the first one with a non-finite input
    int64_t n = a.n_t;
    for (int64_t j0 = 0; j0 < a.n_t; j0 += 64) {
        const int64_t j = j0 + lane;
        bool bad = false;
        if (j < a.n_t)
            bad = !(isfinite(lon[j]) && isfinite(lat[j]) && isfinite(vv[j]) && isfinite(u2[j]) && isfinite(v2[j]) && isfinite(u8[j]) &&
                    isfinite(v8[j]));
        const unsigned long long m = __ballot(bad);
        if (m) { n = j0 + __ffsll((long long)m) - 1; break; }
    }
    WfStage *st = a.stage + s * a.n_t;
    WfRec *row = a.rec + s * a.n_seg_max * kHzSeg;
    // per sample: position, intensity, rm and A, with the neighbour and end-extrapolation rules of k_emit
    bool bad_rm = false;
    if (n >= 2) {
        for (int64_t k = lane; k < n; k += 64) {
            const double x = lon[k], y = lat[k], v = vv[k];
            double lom = 0.0, lam = 0.0, lop = 0.0, lap = 0.0;
            if (k > 0) { lom = lon[k - 1]; lam = lat[k - 1]; }
            if (k < n - 1) { lop = lon[k + 1]; lap = lat[k + 1]; }
            const double lop_in = lop, lap_in = lap, lom_in = lom, lam_in = lam;
            if (k == 0) { lom = 2.0 * x - lop_in; lam = 2.0 * y - lap_in; }
            if (k == n - 1) { lop = 2.0 * x - lom_in; lap = 2.0 * y - lam_in; }
            double ae, an;
            wf_asym(a.dt, y, v, u2[k] - u8[k], v2[k] - v8[k], lom, lam, lop, lap, ae, an);
            const double rm = a.rmax ? a.rmax[o + k] : (a.rm_const > 0.0 ? a.rm_const : 46.4 * exp(-0.0155 * v + 0.0169 * fabs(y)));
            if (!(isfinite(rm) && rm > 0.0)) bad_rm = true;
            st[k] = WfStage{x, y, v, rm, ae, an, 0.0, 0.0};
        }
    }
    const bool drop = __ballot(bad_rm) != 0;
    const int nr = (n >= 2 && !drop) ? (int)((n - 1) * a.sub + 1) : 0;
    __syncthreads();                                    // the records read stage entries other lanes wrote
    for (int q = lane; q < nr; q += 64) {
        const int k = q / a.sub, j = q - k * a.sub;
        const WfStage p = st[k];
        if (j == 0) { row[q] = wf_record(p.lon, p.lat, p.v, p.rm, p.ae, p.an); continue; }
        const WfStage p1 = st[k + 1];
        const double tau = (double)j / (double)a.sub;
        double dl = p1.lon - p.lon;
        dl -= 360.0 * floor((dl + 180.0) / 360.0);      // [-180, 180)
        row[q] = wf_record(p.lon + tau * dl, p.lat + tau * (p1.lat - p.lat), p.v + tau * (p1.v - p.v), p.rm + tau * (p1.rm - p.rm),
                           p.ae + tau * (p1.ae - p.ae), p.an + tau * (p1.an - p.an));
    }
    // the rest of the last segment: records no distance test passes (NaN terms)
    for (int q = nr + lane; q < (nr + kHzSeg - 1) / kHzSeg * kHzSeg; q += 64) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        row[q] = WfRec{nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan};
    }
    __syncthreads();                                    // the caps read records other lanes wrote
    if (lane == 0) a.cnt[s] = nr;
    if (nr == 0) return;
    wf_cap(row, 0, nr, a.storm + s);
    for (int k = 0; k * kHzSeg < nr; ++k) wf_cap(row, k * kHzSeg, min(nr, (k + 1) * kHzSeg), a.seg + s * a.n_seg_max + k);
}

template <bool UNIT_C>
__global__ __launch_bounds__(64) void k_wind_main(WfMainArgs a)
{
    extern __shared__ int32_t hist[];                   // [n_bin + 1][64]: storms of this lane whose max passes exactly k thresholds
    const int lane = threadIdx.x;
    const int64_t tile = blockIdx.x % a.n_tile, chunk = blockIdx.x / a.n_tile;
    const int64_t site = tile * 64 + lane;
    const bool valid = site < a.n_site;
    const int64_t site0 = tile * 64;
    const int64_t my = valid ? site : site0;
    const double y = a.site_lat[my], x = a.site_lon[my];
    const double hp = y * (kPi / 360.0), hl = x * (kPi / 360.0), phi = y * (kPi / 180.0), lam = x * (kPi / 180.0);
    const double sp = sin(hp), cp = cos(hp), sl = sin(hl), cl = cos(hl), cosp = cos(phi);
    const double sinp = sin(phi), sinl = sin(lam), cosl = cos(lam);
    for (int k = 0; k <= a.n_bin; ++k) hist[k * 64 + lane] = 0;

    // tile cap: centre = the tile's first site, radius = the largest angle from it, padded by r_out
    const double sp0 = __shfl(sp, 0, 64), cp0 = __shfl(cp, 0, 64), sl0 = __shfl(sl, 0, 64), cl0 = __shfl(cl, 0, 64);
    const double cosp0 = __shfl(cosp, 0, 64);
    const double rt = wave_max(hz_angle(hz_a(sp0, cp0, sl0, cl0, cosp0, sp, cp, sl, cl, cosp))) + kHzPad + a.r_ang + kHzPad;
    const double phi0 = __shfl(y, 0, 64) * (kPi / 180.0), lam0 = __shfl(x, 0, 64) * (kPi / 180.0);
    const double tx = cos(phi0) * cos(lam0), ty = cos(phi0) * sin(lam0), tz = sin(phi0);
    const double ct = cos(rt), st = sin(rt);

    const int64_t s_begin = hz_uniform(a.chunks + 3 * chunk), s_end = hz_uniform(a.chunks + 3 * chunk + 1);
    const unsigned long long n_lanes = (unsigned long long)min<int64_t>(64, a.n_site - site0);
    unsigned long long pairs = 0;
    __syncthreads();
    for (int64_t s = s_begin; s < s_end; ++s) {
        double m = NAN;
        const int n = hz_uniform(a.cnt + s);
        if (n > 0 && !hz_far(hz_uniform(a.storm + s), tx, ty, tz, ct, st, rt)) {
            const WfRec *row = a.rec + s * a.n_seg_max * kHzSeg;
            const HzCap *segs = a.seg + s * a.n_seg_max;
            for (int k = 0; k * kHzSeg < n; ++k) {
                if (hz_far(hz_uniform(segs + k), tx, ty, tz, ct, st, rt)) continue;
                pairs += (unsigned long long)(min(n, (k + 1) * kHzSeg) - k * kHzSeg);
                const WfRec *seg = row + k * kHzSeg;
#pragma unroll 2
                for (int j = 0; j < kHzSeg; ++j) {              // (padding records fail the test: NaN terms)
                    const WfRec p = wf_uniform(seg + j);
                    const double q = hz_a(sp, cp, sl, cl, cosp, p.sp, p.cp, p.sl, p.cl, p.cosp);
                    if (q <= a.a_out) {
                        const double r = (2.0 * asin(sqrt(q))) * kWfEarthR;
                        double V;
                        if (UNIT_C) {
                            V = r * (2.0 * p.mm / (p.rm * p.rm + r * r) - p.f2);
                        } else {
                            const double xr = r / p.rm, x2 = xr * xr;
                            V = r > 0.0 ? (p.mm * pow(2.0 * x2 / (a.two_c + a.c * x2), a.inv_exp) - p.f2 * (r * r)) / r : 0.0;
                        }
                        V = fmax(V, 0.0);
                        const double sdl = sinl * p.cosl - cosl * p.sinl, cdl = cosl * p.cosl + sinl * p.sinl;
                        const double e = cosp * sdl, nn = p.cosp * sinp - p.sinp * (cosp * cdl);
                        const double dd = e * e + nn * nn;
                        const double cross = dd > 0.0 ? (e * p.bn - nn * p.be) / sqrt(dd) : 0.0;
                        m = fmax(m, V * sqrt(p.a2 + cross));    // fmax skips the NaN start
                    }
                }
            }
        }
        if (a.site_max && valid) a.site_max[site * a.n_trk + s] = m;
        if (!isnan(m)) {
            int lo = 0, hi = a.n_bin;                   // k = #thresholds <= m
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.thr[mid] <= m) lo = mid + 1; else hi = mid; }
            hist[lo * 64 + lane] += 1;
        }
    }
    if (valid) {
        int32_t c = 0;
        int32_t *out = a.part + (chunk * a.n_site + site) * a.n_bin;
        for (int b = a.n_bin - 1; b >= 0; --b) { c += hist[(b + 1) * 64 + lane]; out[b] = c; }
    }
    if (lane == 0 && pairs) atomicAdd(a.pairs, pairs * n_lanes);
}

template <typename T>
int wf_grow(tcr_ctx *ctx, int i, size_t count)
{
    if (ctx->wf_cap[i] >= count * sizeof(T)) return 0;
    (void)hipFree(ctx->d_wf[i]);
    ctx->d_wf[i] = nullptr; ctx->wf_cap[i] = 0;
    T *p = nullptr;
    if (dev_alloc(ctx, &p, count)) return -1;
    ctx->d_wf[i] = p; ctx->wf_cap[i] = count * sizeof(T);
    return 0;
}

int windfield_check(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *p, int64_t n_site, const double *site_lon,
                    const double *site_lat, int32_t n_bin, const double *thr, const int32_t *counts)
{
    if (!t || !p || !site_lon || !site_lat || !thr || !counts || !t->lon || !t->lat || !t->v || !t->u250 || !t->v250 || !t->u850 ||
        !t->v850 || !t->group_off)
        return fail(ctx, "tcr_windfield: NULL argument");
    if (!(p->dt_s > 0.0 && std::isfinite(p->dt_s))) return fail(ctx, "tcr_windfield: dt_s must be finite and > 0");
    if (!(p->ck_cd > 0.0 && p->ck_cd < 2.0)) return fail(ctx, "tcr_windfield: ck_cd must be in (0, 2)");
    if (!(p->r_out_km > 0.0 && p->r_out_km <= 2000.0)) return fail(ctx, "tcr_windfield: r_out_km must be in (0, 2000]");
    if (p->substeps < 1 || p->substeps > kWfMaxSub) return fail(ctx, "tcr_windfield: substeps must be in [1, 64]");
    if (!(p->rmax_const_km >= 0.0 && std::isfinite(p->rmax_const_km)) || (t->rmax_km && p->rmax_const_km != 0.0))
        return fail(ctx, "tcr_windfield: rmax_const_km must be finite and >= 0, and 0 when the rmax_km plane is given");
    if (n_bin < 1 || n_bin > kHzMaxBin) return fail(ctx, "tcr_windfield: n_bin must be in [1, 64]");
    for (int b = 0; b < n_bin; ++b)
        if (!std::isfinite(thr[b]) || (b > 0 && !(thr[b] > thr[b - 1]))) return fail(ctx, "tcr_windfield: thresholds must be finite and ascending");
    if (n_site < 1 || t->n_trk < 0 || t->n_t < 1 || t->n_t > (1 << 20) || t->row_stride < t->n_t || t->n_group < 1)
        return fail(ctx, "tcr_windfield: bad sizes (n_site >= 1, 1 <= n_t <= 2^20, row_stride >= n_t, n_group >= 1)");
    if (t->group_off[0] != 0 || t->group_off[t->n_group] != t->n_trk) return fail(ctx, "tcr_windfield: group_off must run from 0 to n_trk");
    for (int32_t g = 0; g < t->n_group; ++g)
        if (t->group_off[g + 1] < t->group_off[g]) return fail(ctx, "tcr_windfield: group_off must not decrease");
    return 0;
}

}  // namespace

extern "C" {

int tcr_windfield_dev(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                      const double *site_lat, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max, void *stream_)
{
    if (!ctx) return -1;
    if (windfield_check(ctx, t, prm, n_site, site_lon, site_lat, n_bin, thresholds, counts)) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_ ? (hipStream_t)stream_ : ctx->stream;
    const int64_t n_trk = t->n_trk, n_t = t->n_t, n_group = t->n_group, sub = prm->substeps;
    const int64_t n_tile = (n_site + 63) / 64, n_seg_max = ((n_t - 1) * sub + 1 + kHzSeg - 1) / kHzSeg;

    // chunks: every group split into pieces of at most `ch` storms, sized so that the grid has ~8192 waves (as the hazard)
    const int64_t want = std::max<int64_t>(1, (8192 + n_tile - 1) / n_tile);
    const int64_t ch = std::max<int64_t>(16, (n_trk + want - 1) / want);
    std::vector<int64_t> tab, gch(1, 0);
    for (int64_t g = 0; g < n_group; ++g) {
        for (int64_t b = t->group_off[g]; b < t->group_off[g + 1]; b += ch) {
            tab.push_back(b); tab.push_back(std::min(b + ch, (int64_t)t->group_off[g + 1])); tab.push_back(g);
        }
        gch.push_back((int64_t)tab.size() / 3);
    }
    const int64_t n_chunk = (int64_t)tab.size() / 3;
    if (n_tile * n_chunk >= ((int64_t)1 << 31) || n_site * n_group * n_bin >= ((int64_t)1 << 39))
        return fail(ctx, "tcr_windfield: too many sites x storm chunks for one launch; split the sites");
    const size_t n_tab = tab.size() + gch.size();

    if (wf_grow<WfRec>(ctx, 0, (size_t)std::max<int64_t>(1, n_trk * n_seg_max * kHzSeg)) ||
        wf_grow<HzCap>(ctx, 1, (size_t)std::max<int64_t>(1, n_trk * (n_seg_max + 1))) ||
        wf_grow<int32_t>(ctx, 2, (size_t)std::max<int64_t>(1, n_trk)) ||
        wf_grow<int32_t>(ctx, 3, (size_t)std::max<int64_t>(1, n_chunk * n_site * n_bin)) ||
        wf_grow<int64_t>(ctx, 4, n_tab + 1) ||
        wf_grow<WfStage>(ctx, 5, (size_t)std::max<int64_t>(1, n_trk * n_t)))
        return -1;
    // the chunk table goes up through a pinned buffer of the context; the previous call's upload must be done with it
    if (ctx->wf_ev) HIPCHK(ctx, hipEventSynchronize(ctx->wf_ev));
    else {
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->wf_ev, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->wf_done, hipEventDisableTiming));
    }
    if (ctx->wf_h_cap < n_tab) {
        if (ctx->wf_h) (void)hipHostFree(ctx->wf_h);
        ctx->wf_h = nullptr; ctx->wf_h_cap = 0;
        HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->wf_h), n_tab * sizeof(int64_t)));
        ctx->wf_h_cap = n_tab;
    }
    memcpy(ctx->wf_h, tab.data(), tab.size() * sizeof(int64_t));
    memcpy(ctx->wf_h + tab.size(), gch.data(), gch.size() * sizeof(int64_t));
    int64_t *d_tab = static_cast<int64_t *>(ctx->d_wf[4]);
    unsigned long long *d_pairs = reinterpret_cast<unsigned long long *>(d_tab + n_tab);
    HIPCHK(ctx, hipMemcpyAsync(d_tab, ctx->wf_h, n_tab * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(ctx->wf_ev, st));
    HIPCHK(ctx, hipMemsetAsync(d_pairs, 0, sizeof(unsigned long long), st));
    ctx->wf_pairs = d_pairs;

    WfRec *rec = static_cast<WfRec *>(ctx->d_wf[0]);
    HzCap *caps = static_cast<HzCap *>(ctx->d_wf[1]);
    int32_t *cnt = static_cast<int32_t *>(ctx->d_wf[2]), *part = static_cast<int32_t *>(ctx->d_wf[3]);
    if (n_trk > 0) {
        WfPrepArgs p{t->lon, t->lat, t->v, t->u250, t->v250, t->u850, t->v850, t->rmax_km, n_trk, n_t, t->row_stride,
                     prm->dt_s, prm->rmax_const_km, (int32_t)sub, static_cast<WfStage *>(ctx->d_wf[5]), rec, caps + n_trk, caps, cnt,
                     n_seg_max};
        hipLaunchKernelGGL(k_wind_prep, dim3((unsigned)n_trk), dim3(64), 0, st, p);
        HIPCHK(ctx, hipGetLastError());
    }
    if (n_chunk > 0) {
        WfMainArgs m{};
        m.rec = rec; m.seg = caps + n_trk; m.storm = caps; m.cnt = cnt; m.chunks = d_tab;
        m.site_lon = site_lon; m.site_lat = site_lat;
        m.n_site = n_site; m.n_tile = n_tile; m.n_seg_max = n_seg_max; m.n_trk = n_trk;
        const double re_km = kWfEarthR / 1000.0, h = sin(prm->r_out_km / (2.0 * re_km));
        m.a_out = h * h; m.r_ang = prm->r_out_km / re_km;
        m.c = prm->ck_cd; m.two_c = 2.0 - prm->ck_cd; m.inv_exp = 1.0 / (2.0 - prm->ck_cd);
        m.n_bin = n_bin;
        for (int b = 0; b < n_bin; ++b) m.thr[b] = thresholds[b];
        m.part = part; m.site_max = site_max; m.pairs = d_pairs;
        const size_t lds = sizeof(int32_t) * 64 * (n_bin + 1);
        if (prm->ck_cd == 1.0) hipLaunchKernelGGL(k_wind_main<true>, dim3((unsigned)(n_tile * n_chunk)), dim3(64), lds, st, m);
        else hipLaunchKernelGGL(k_wind_main<false>, dim3((unsigned)(n_tile * n_chunk)), dim3(64), lds, st, m);
        HIPCHK(ctx, hipGetLastError());
    }
    const int64_t n_out = n_site * n_group * n_bin;
    hipLaunchKernelGGL(k_hazard_reduce, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, part, d_tab + tab.size(), n_site,
                       (int32_t)n_group, n_bin, counts);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->wf_done, st));
    return 0;
}

int tcr_windfield_host(tcr_ctx *ctx, const tcr_wind_tracks *t, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                       const double *site_lat, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max)
{
    if (!ctx) return -1;
    if (windfield_check(ctx, t, prm, n_site, site_lon, site_lat, n_bin, thresholds, counts)) return -1;
    // rm > 0 and finite at every sample of a track (the device entry point cannot report it)
    if (t->rmax_km) {
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
                if (!(std::isfinite(t->rmax_km[o + k]) && t->rmax_km[o + k] > 0.0))
                    return fail(ctx, "tcr_windfield_host: rmax_km must be finite and > 0 at every sample of a track");
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf B;
    const size_t plane = (size_t)std::max<int64_t>(1, t->n_trk * t->row_stride);
    tcr_wind_tracks d = *t;
    d.lon = B.put(t->lon, plane); d.lat = B.put(t->lat, plane); d.v = B.put(t->v, plane);
    d.u250 = B.put(t->u250, plane); d.v250 = B.put(t->v250, plane); d.u850 = B.put(t->u850, plane); d.v850 = B.put(t->v850, plane);
    d.rmax_km = t->rmax_km ? B.put(t->rmax_km, plane) : nullptr;
    const double *d_slon = B.put(site_lon, (size_t)n_site), *d_slat = B.put(site_lat, (size_t)n_site);
    const size_t n_out = (size_t)n_site * t->n_group * n_bin, n_max = (size_t)n_site * std::max<int64_t>(1, t->n_trk);
    int32_t *d_counts = B.get<int32_t>(n_out);
    double *d_max = site_max ? B.get<double>(n_max) : nullptr;
    if (!d.lon || !d.lat || !d.v || !d.u250 || !d.v250 || !d.u850 || !d.v850 || (t->rmax_km && !d.rmax_km) || !d_slon || !d_slat ||
        !d_counts || (site_max && !d_max))
        return fail(ctx, "tcr_windfield_host: device allocation / upload failed");
    if (tcr_windfield_dev(ctx, &d, prm, n_site, d_slon, d_slat, n_bin, thresholds, d_counts, d_max, ctx->stream)) return -1;
    HIPCHK(ctx, hipMemcpyAsync(counts, d_counts, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost, ctx->stream));
    if (site_max) HIPCHK(ctx, hipMemcpyAsync(site_max, d_max, sizeof(double) * (size_t)n_site * t->n_trk, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int tcr_windfield_pairs(tcr_ctx *ctx, int64_t *pairs)
{
    if (!ctx) return -1;
    if (!pairs) return fail(ctx, "tcr_windfield_pairs: NULL argument");
    if (!ctx->wf_pairs) return fail(ctx, "tcr_windfield_pairs: no tcr_windfield_* call on this context yet");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned long long v = 0;
    HIPCHK(ctx, hipEventSynchronize(ctx->wf_done));
    HIPCHK(ctx, copy_sync(ctx->stream, &v, ctx->wf_pairs, sizeof v, hipMemcpyDeviceToHost));
    *pairs = (int64_t)v;
    return 0;
}

}  // extern "C"
