// Site wind hazard behind the C ABI (include/tcrisk_hip.h, "site hazard" section): the analysis the reference's
// notebooks/sample_analysis.ipynb runs on a track file, for many sites at once.
//
//   max[site][storm] = nanmax of vmax over the samples with haversine(site, sample) <= R   (NaN when there are none)
//   counts[site][group][bin] = #storms of the group with max >= thr[bin]
//
// Three kernels:
//   k_hazard_prep    one wave per storm: compacts the live samples (lon and lat not NaN) to the front of the storm's row as
//                    { sin(phi/2), cos(phi/2), sin(lam/2), cos(lam/2), cos(phi), vmax, lat, lon }, and writes a bounding cap
//                    (unit-vector centre, angular radius) of the storm and of every kHzSeg-sample segment of it;
//   k_hazard_main    one wave per (tile of 64 sites, chunk of storms of one group): every lane holds one site's terms in
//                    registers; the storm samples are wave-uniform and come through scalar loads.  A storm or segment whose cap
//                    is farther than R (plus both radii) from the tile's cap is skipped without touching its samples;
//   k_hazard_reduce  sums the integer per-chunk partial counts of each group.
//
// The distance decision.  The notebook's d = 6378 * 2 * arcsin(sqrt(a)), a = sin^2(dphi/2) + cos phi1 cos phi2 sin^2(dlam/2), is
// monotone in a, so d <= R is a <= a_R = sin^2(R / (2 * 6378)) (a_R computed once on the host).  sin(dphi/2) and sin(dlam/2) are
// formed by the difference identity from the per-point half-angle terms: no trigonometry per pair, and the form is periodic in 360
// degrees of longitude, so sites and tracks may use different conventions.  At 100 km it differs from NumPy's d by ~5e-12 km.
//
// Culling is conservative: caps are padded by kHzPad radians and the test keeps a margin of kHzDotPad in cosine space (both far above
// the rounding of the cap arithmetic), so a skipped pair is always farther than R.  It changes which pairs are evaluated, never a
// result: max is a max of inputs (no arithmetic) and the counts are integers, so results are bit-identical whatever the launch shape.

namespace {

constexpr int kHzSeg = 32;                  // samples per culling segment
constexpr int kHzMaxBin = 64;
constexpr double kHzRe = 6378.0;            // r_earth of the notebook's haversine (km)
constexpr double kHzPad = 1e-9;             // radians added to every cap radius
constexpr double kHzDotPad = 1e-12;         // cosine-space margin of the cap test

struct HzSample { double sp, cp, sl, cl, cosp, v, lat, lon; };     // one live sample (64 bytes)
struct HzCap { double x, y, z, cr, sr, r, pad0, pad1; };           // cap: centre, cos / sin of radius, radius (64 bytes)

struct HzPrepArgs {
    const double *lon, *lat, *vmax;
    int64_t n_trk, n_t, stride;
    HzSample *smp;                          // [n_trk][n_seg_max * kHzSeg]
    HzCap *seg;                             // [n_trk][n_seg_max]
    HzCap *storm;                           // [n_trk]
    int32_t *cnt;                           // [n_trk] live samples
    int64_t n_seg_max;
};

struct HzMainArgs {
    const HzSample *smp;
    const HzCap *seg, *storm;
    const int32_t *cnt;
    const int64_t *chunks;                  // [n_chunk][3]: storm begin, storm end, group
    const double *site_lon, *site_lat;
    int64_t n_site, n_tile, n_seg_max, n_trk;
    double a_R, r_ang;                      // a threshold, R in radians
    int32_t n_bin;
    double thr[kHzMaxBin];
    int32_t *part;                          // [n_chunk][n_site][n_bin]
    double *site_max;                       // [n_site][n_trk] or NULL
    unsigned long long *pairs;              // pairs evaluated (after culling)
};

// Wave-uniform reads of data no kernel here writes while it runs: through the constant address space, so that the compiler issues
// scalar loads (the values then feed the fp64 VALU as SGPR operands) instead of vector loads of one address per lane.
template <typename T>
__device__ __forceinline__ T hz_uniform(const T *p) { return *(const __attribute__((address_space(4))) T *)p; }
__device__ __forceinline__ HzSample hz_uniform(const HzSample *p)
{
    const double *d = &p->sp;
    return HzSample{hz_uniform(d), hz_uniform(d + 1), hz_uniform(d + 2), hz_uniform(d + 3), hz_uniform(d + 4), hz_uniform(d + 5), 0.0, 0.0};
}
__device__ __forceinline__ HzCap hz_uniform(const HzCap *p)
{
    const double *d = &p->x;
    return HzCap{hz_uniform(d), hz_uniform(d + 1), hz_uniform(d + 2), hz_uniform(d + 3), hz_uniform(d + 4), hz_uniform(d + 5), 0.0, 0.0};
}

__device__ __forceinline__ double hz_a(double sp1, double cp1, double sl1, double cl1, double cosp1,
                                       double sp2, double cp2, double sl2, double cl2, double cosp2)
{
    const double t1 = sp1 * cp2 - cp1 * sp2;     // sin((phi1 - phi2) / 2)
    const double t2 = sl1 * cl2 - cl1 * sl2;     // sin((lam1 - lam2) / 2)
    return t1 * t1 + (cosp1 * cosp2) * (t2 * t2);
}

__device__ __forceinline__ double hz_angle(double a) { return 2.0 * asin(sqrt(fmin(fmax(a, 0.0), 1.0))); }

__device__ __forceinline__ double wave_max(double x)
{
    for (int o = 32; o >= 1; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

// cap (centre = the sample at `mid`, radius = the largest angle from it) of the samples [b, e) of one row
__device__ void hz_cap(const HzSample *row, int b, int e, HzCap *out)
{
    const int lane = threadIdx.x;
    const HzSample &c = row[b + (e - b) / 2];
    double r = 0.0;
    for (int j = b + lane; j < e; j += 64) {
        const HzSample &p = row[j];
        r = fmax(r, hz_angle(hz_a(c.sp, c.cp, c.sl, c.cl, c.cosp, p.sp, p.cp, p.sl, p.cl, p.cosp)));
    }
    r = wave_max(r) + kHzPad;
    if (lane == 0) {
        const double phi = c.lat * (M_PI / 180.0), lam = c.lon * (M_PI / 180.0);
        out->x = cos(phi) * cos(lam); out->y = cos(phi) * sin(lam); out->z = sin(phi);
        out->cr = cos(r); out->sr = sin(r); out->r = r; out->pad0 = out->pad1 = 0.0;
    }
}

__global__ __launch_bounds__(64) void k_hazard_prep(HzPrepArgs a)
{
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const double *lon = a.lon + s * a.stride, *lat = a.lat + s * a.stride, *vm = a.vmax + s * a.stride;
    HzSample *row = a.smp + s * a.n_seg_max * kHzSeg;
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
    // the rest of the last segment: samples no distance test passes (NaN terms), so that every segment is kHzSeg samples long
    for (int j = n + lane; j < (n + kHzSeg - 1) / kHzSeg * kHzSeg; j += 64) row[j] = HzSample{NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN};
    __syncthreads();                                    // the caps read samples other lanes wrote
    if (lane == 0) a.cnt[s] = n;
    if (n == 0) return;
    hz_cap(row, 0, n, a.storm + s);
    for (int k = 0; k * kHzSeg < n; ++k) hz_cap(row, k * kHzSeg, min(n, (k + 1) * kHzSeg), a.seg + s * a.n_seg_max + k);
}

// true when no point of the cap can be within the tile's padded radius (cos_t, sin_t, r_t) of the tile centre (tx, ty, tz)
__device__ __forceinline__ bool hz_far(const HzCap &c, double tx, double ty, double tz, double ct, double st, double rt)
{
    if (c.r + rt >= M_PI) return false;
    const double dot = c.x * tx + c.y * ty + c.z * tz;
    return dot < c.cr * ct - c.sr * st - kHzDotPad;     // angle(centres) > r_cap + r_tile
}

__global__ __launch_bounds__(64) void k_hazard_main(HzMainArgs a)
{
    extern __shared__ int32_t hist[];                   // [n_bin + 1][64]: storms of this lane whose max passes exactly k thresholds
    const int lane = threadIdx.x;
    const int64_t tile = blockIdx.x % a.n_tile, chunk = blockIdx.x / a.n_tile;
    const int64_t site = tile * 64 + lane;
    const bool valid = site < a.n_site;
    const int64_t site0 = tile * 64;
    const int64_t my = valid ? site : site0;
    const double y = a.site_lat[my], x = a.site_lon[my];
    const double hp = y * (M_PI / 360.0), hl = x * (M_PI / 360.0);
    const double sp = sin(hp), cp = cos(hp), sl = sin(hl), cl = cos(hl), cosp = cos(y * (M_PI / 180.0));
    for (int k = 0; k <= a.n_bin; ++k) hist[k * 64 + lane] = 0;

    // tile cap: centre = the tile's first site, radius = the largest angle from it, padded by R
    const double sp0 = __shfl(sp, 0, 64), cp0 = __shfl(cp, 0, 64), sl0 = __shfl(sl, 0, 64), cl0 = __shfl(cl, 0, 64);
    const double cosp0 = __shfl(cosp, 0, 64);
    const double rt = wave_max(hz_angle(hz_a(sp0, cp0, sl0, cl0, cosp0, sp, cp, sl, cl, cosp))) + kHzPad + a.r_ang + kHzPad;
    const double phi0 = __shfl(y, 0, 64) * (M_PI / 180.0), lam0 = __shfl(x, 0, 64) * (M_PI / 180.0);
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
            const HzSample *row = a.smp + s * a.n_seg_max * kHzSeg;
            const HzCap *segs = a.seg + s * a.n_seg_max;
            for (int k = 0; k * kHzSeg < n; ++k) {
                if (hz_far(hz_uniform(segs + k), tx, ty, tz, ct, st, rt)) continue;
                pairs += (unsigned long long)(min(n, (k + 1) * kHzSeg) - k * kHzSeg);
                const HzSample *seg = row + k * kHzSeg;
#pragma unroll 4
                for (int j = 0; j < kHzSeg; ++j) {                  // (padding samples fail the test: NaN terms)
                    const HzSample p = hz_uniform(seg + j);
                    if (hz_a(sp, cp, sl, cl, cosp, p.sp, p.cp, p.sl, p.cl, p.cosp) <= a.a_R) m = fmax(m, p.v);   // fmax skips NaN
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

// counts[site][g][b] = sum of the partials of the chunks of group g
__global__ __launch_bounds__(256) void k_hazard_reduce(const int32_t *__restrict__ part, const int64_t *__restrict__ gch_off,
                                                       int64_t n_site, int32_t n_group, int32_t n_bin, int32_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_site * n_group * n_bin) return;
    const int64_t b = i % n_bin, g = (i / n_bin) % n_group, site = i / ((int64_t)n_bin * n_group);
    int32_t c = 0;
    for (int64_t k = gch_off[g]; k < gch_off[g + 1]; ++k) c += part[(k * n_site + site) * n_bin + b];
    counts[i] = c;
}

template <typename T>
int hz_grow(tcr_ctx *ctx, int i, size_t count)
{
    if (ctx->hz_cap[i] >= count * sizeof(T)) return 0;
    (void)hipFree(ctx->d_hz[i]);
    ctx->d_hz[i] = nullptr; ctx->hz_cap[i] = 0;
    T *p = nullptr;
    if (dev_alloc(ctx, &p, count)) return -1;
    ctx->d_hz[i] = p; ctx->hz_cap[i] = count * sizeof(T);
    return 0;
}

int hazard_check(tcr_ctx *ctx, const tcr_hazard_tracks *t, int64_t n_site, const double *site_lon, const double *site_lat,
                 double radius_km, int32_t n_bin, const double *thr, const int32_t *counts)
{
    if (!t || !site_lon || !site_lat || !thr || !counts || !t->lon || !t->lat || !t->vmax || !t->group_off)
        return fail(ctx, "tcr_hazard: NULL argument");
    if (!(radius_km > 0.0 && radius_km <= 5000.0)) return fail(ctx, "tcr_hazard: radius_km must be in (0, 5000]");
    if (n_bin < 1 || n_bin > kHzMaxBin) return fail(ctx, "tcr_hazard: n_bin must be in [1, 64]");
    for (int b = 0; b < n_bin; ++b)
        if (!std::isfinite(thr[b]) || (b > 0 && !(thr[b] > thr[b - 1]))) return fail(ctx, "tcr_hazard: thresholds must be finite and ascending");
    if (n_site < 1 || t->n_trk < 0 || t->n_t < 1 || t->row_stride < t->n_t || t->n_group < 1)
        return fail(ctx, "tcr_hazard: bad sizes (n_site >= 1, n_t >= 1, row_stride >= n_t, n_group >= 1)");
    if (t->group_off[0] != 0 || t->group_off[t->n_group] != t->n_trk) return fail(ctx, "tcr_hazard: group_off must run from 0 to n_trk");
    for (int32_t g = 0; g < t->n_group; ++g)
        if (t->group_off[g + 1] < t->group_off[g]) return fail(ctx, "tcr_hazard: group_off must not decrease");
    return 0;
}

}  // namespace

extern "C" {

int tcr_hazard_dev(tcr_ctx *ctx, const tcr_hazard_tracks *t, int64_t n_site, const double *site_lon, const double *site_lat,
                   double radius_km, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max, void *stream_)
{
    if (!ctx) return -1;
    if (hazard_check(ctx, t, n_site, site_lon, site_lat, radius_km, n_bin, thresholds, counts)) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_ ? (hipStream_t)stream_ : ctx->stream;
    const int64_t n_trk = t->n_trk, n_t = t->n_t, n_group = t->n_group;
    const int64_t n_tile = (n_site + 63) / 64, n_seg_max = (n_t + kHzSeg - 1) / kHzSeg;

    // chunks: every group split into pieces of at most `ch` storms, sized so that the grid has ~8192 waves
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
        return fail(ctx, "tcr_hazard: too many sites x storm chunks for one launch; split the sites");
    const size_t n_tab = tab.size() + gch.size();

    if (hz_grow<HzSample>(ctx, 0, (size_t)std::max<int64_t>(1, n_trk * n_seg_max * kHzSeg)) ||
        hz_grow<HzCap>(ctx, 1, (size_t)std::max<int64_t>(1, n_trk * (n_seg_max + 1))) ||
        hz_grow<int32_t>(ctx, 2, (size_t)std::max<int64_t>(1, n_trk)) ||
        hz_grow<int32_t>(ctx, 3, (size_t)std::max<int64_t>(1, n_chunk * n_site * n_bin)) ||
        hz_grow<int64_t>(ctx, 4, n_tab + 1))
        return -1;
    // the chunk table goes up through a pinned buffer of the context; the previous call's upload must be done with it
    if (ctx->hz_ev) HIPCHK(ctx, hipEventSynchronize(ctx->hz_ev));
    else {
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->hz_ev, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->hz_done, hipEventDisableTiming));
    }
    if (ctx->hz_h_cap < n_tab) {
        if (ctx->hz_h) (void)hipHostFree(ctx->hz_h);
        ctx->hz_h = nullptr; ctx->hz_h_cap = 0;
        HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->hz_h), n_tab * sizeof(int64_t)));
        ctx->hz_h_cap = n_tab;
    }
    memcpy(ctx->hz_h, tab.data(), tab.size() * sizeof(int64_t));
    memcpy(ctx->hz_h + tab.size(), gch.data(), gch.size() * sizeof(int64_t));
    int64_t *d_tab = static_cast<int64_t *>(ctx->d_hz[4]);
    unsigned long long *d_pairs = reinterpret_cast<unsigned long long *>(d_tab + n_tab);
    HIPCHK(ctx, hipMemcpyAsync(d_tab, ctx->hz_h, n_tab * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(ctx->hz_ev, st));
    HIPCHK(ctx, hipMemsetAsync(d_pairs, 0, sizeof(unsigned long long), st));
    ctx->hz_pairs = d_pairs;

    HzSample *smp = static_cast<HzSample *>(ctx->d_hz[0]);
    HzCap *caps = static_cast<HzCap *>(ctx->d_hz[1]);
    int32_t *cnt = static_cast<int32_t *>(ctx->d_hz[2]), *part = static_cast<int32_t *>(ctx->d_hz[3]);
    if (n_trk > 0) {
        HzPrepArgs p{t->lon, t->lat, t->vmax, n_trk, n_t, t->row_stride, smp, caps + n_trk, caps, cnt, n_seg_max};
        hipLaunchKernelGGL(k_hazard_prep, dim3((unsigned)n_trk), dim3(64), 0, st, p);
        HIPCHK(ctx, hipGetLastError());
    }
    if (n_chunk > 0) {
        HzMainArgs m{};
        m.smp = smp; m.seg = caps + n_trk; m.storm = caps; m.cnt = cnt; m.chunks = d_tab;
        m.site_lon = site_lon; m.site_lat = site_lat;
        m.n_site = n_site; m.n_tile = n_tile; m.n_seg_max = n_seg_max; m.n_trk = n_trk;
        const double h = sin(radius_km / (2.0 * kHzRe));
        m.a_R = h * h; m.r_ang = radius_km / kHzRe;
        m.n_bin = n_bin;
        for (int b = 0; b < n_bin; ++b) m.thr[b] = thresholds[b];
        m.part = part; m.site_max = site_max; m.pairs = d_pairs;
        hipLaunchKernelGGL(k_hazard_main, dim3((unsigned)(n_tile * n_chunk)), dim3(64), sizeof(int32_t) * 64 * (n_bin + 1), st, m);
        HIPCHK(ctx, hipGetLastError());
    }
    const int64_t n_out = n_site * n_group * n_bin;
    hipLaunchKernelGGL(k_hazard_reduce, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, part, d_tab + tab.size(), n_site,
                       (int32_t)n_group, n_bin, counts);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->hz_done, st));
    return 0;
}

int tcr_hazard_host(tcr_ctx *ctx, const tcr_hazard_tracks *t, int64_t n_site, const double *site_lon, const double *site_lat,
                    double radius_km, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max)
{
    if (!ctx) return -1;
    if (hazard_check(ctx, t, n_site, site_lon, site_lat, radius_km, n_bin, thresholds, counts)) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf B;
    const size_t plane = (size_t)std::max<int64_t>(1, t->n_trk * t->row_stride);
    tcr_hazard_tracks d = *t;
    d.lon = B.put(t->lon, plane); d.lat = B.put(t->lat, plane); d.vmax = B.put(t->vmax, plane);
    const double *d_slon = B.put(site_lon, (size_t)n_site), *d_slat = B.put(site_lat, (size_t)n_site);
    const size_t n_out = (size_t)n_site * t->n_group * n_bin, n_max = (size_t)n_site * std::max<int64_t>(1, t->n_trk);
    int32_t *d_counts = B.get<int32_t>(n_out);
    double *d_max = site_max ? B.get<double>(n_max) : nullptr;
    if (!d.lon || !d.lat || !d.vmax || !d_slon || !d_slat || !d_counts || (site_max && !d_max))
        return fail(ctx, "tcr_hazard_host: device allocation / upload failed");
    if (tcr_hazard_dev(ctx, &d, n_site, d_slon, d_slat, radius_km, n_bin, thresholds, d_counts, d_max, ctx->stream)) return -1;
    HIPCHK(ctx, hipMemcpyAsync(counts, d_counts, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost, ctx->stream));
    if (site_max) HIPCHK(ctx, hipMemcpyAsync(site_max, d_max, sizeof(double) * (size_t)n_site * t->n_trk, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int tcr_hazard_pairs(tcr_ctx *ctx, int64_t *pairs)
{
    if (!ctx) return -1;
    if (!pairs) return fail(ctx, "tcr_hazard_pairs: NULL argument");
    if (!ctx->hz_pairs) return fail(ctx, "tcr_hazard_pairs: no tcr_hazard_* call on this context yet");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned long long v = 0;
    HIPCHK(ctx, hipEventSynchronize(ctx->hz_done));
    HIPCHK(ctx, copy_sync(ctx->stream, &v, ctx->hz_pairs, sizeof v, hipMemcpyDeviceToHost));
    *pairs = (int64_t)v;
    return 0;
}

}  // extern "C"
