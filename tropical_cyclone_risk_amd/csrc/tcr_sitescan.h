// The site scan: what the per-site analyses of a track ensemble share.  Its users: tcr_hazard.hip, tcr_windfield.hip,
// tcr_loss.hip, tcr_rainfall.hip, tcr_compound.hip, tcr_duration.hip, tcr_directional.hip, tcr_accumulation.hip.  Each of them turns every storm into a
// row of wave-uniform
// records, accumulates something per (site, storm) over the storm's records with haversine(site, record) <= R, and counts the
// storms of every group by what was accumulated.  In the plainest form (ScanPeak below):
//
//   site_max[site][storm] = max of value(site, record) over those records   (NaN: none)
//   counts[site][group][bin] = #storms of the group with site_max >= thr[bin]
//
// An analysis supplies
//   a record type   8-byte slots that begin with the half-angle terms { sp, cp, sl, cl, cosp } of the point (the distance test):
//                   doubles, and int64 for what a prep kernel counts (a half-weight, a record's index), with
//                   static Rec uniform(const Rec *)  (every slot a policy may read, through scalar loads: one that the running
//                   policy does not read is dead code)  and  void centre(HzCap *) const  (the unit vector of the point, for a
//                   cap centred on it);
//   a prep kernel   one wave per storm: writes the storm's records to the front of its row and ends with scan_finish_row
//                   (NaN padding of the last segment, record count, bounding caps of the storm and of every kHzSeg-record segment);
//   a policy        { Rec, Mode, kUnroll, value(site, record, a) and whatever else its mode calls }: a compile-time type that
//                   travels to the kernel by value, so that it can carry launch-uniform parameters.  Nothing here branches at run
//                   time on which analysis is running;
//   a mode          the policy's one accumulator, Policy::Mode: what a lane keeps of a storm and of a chunk, and where it goes.
//                     Mode::Storm                      a lane's state of one storm, default-constructed per storm;
//                     the mode object                  a lane's state over the chunk's storms;
//                     begin(pol, lane)                 zeroes the lane's cells of the wave's LDS (the mode knows how many, and of
//                                                      what type) and loads what the lane needs over the chunk;
//                     add(pol, storm, me, rec, q)      an included pair (q = its haversine argument <= a_R);
//                     end_storm(pol, lane, storm, s, near)   every lane of the wave calls it, once per storm s, included records
//                                                      or not (near: the storm's cap reaches the tile, wave-uniform): the
//                                                      per-storm outputs and the storm's place in the lane's histogram;
//                     end_chunk(pol, lane)             the lane's n_cell partial counts of this chunk, and its per-chunk totals;
//                     on the host  a ScanShape: the partial counts of a (chunk, site), the LDS bytes of a wave, the thresholds.
//                   Here: ScanStack, the histogram of up to kScanMaxRow values per storm, each with an optional plane and
//                   (n_hbin + 1) cells of its own, and on it ScanPeak<false> (max) and ScanPeak<true> (sum in record order), its
//                   one-row case.  A mode only one analysis has is in that analysis's file, with its own argument for what
//                   follows: LossMode (tcr_loss.hip, on ScanPeak), ScanJoint (tcr_compound.hip), and on ScanStack ScanLevels
//                   (tcr_duration.hip), ScanSectors (tcr_directional.hip) and ScanWindows (tcr_accumulation.hip).
// and calls scan_run with a ScanPlan and a workspace of its own (ScanWs, one instance per user in tcr_ctx: calls of different
// analyses may be in flight on different streams of one context).
//
//   k_site_scan      one wave per (tile of 64 sites, chunk of storms of one group): every lane holds one site's terms in registers;
//                    the records are wave-uniform and come through scalar loads.  A storm or segment whose cap is farther than R
//                    (plus both radii) from the tile's cap is skipped without touching its records;
//   k_hazard_reduce  sums the integer per-chunk partial counts of each group.
//
// Culling is conservative: caps are padded by kHzPad radians and the test keeps a margin of kHzDotPad in cosine space (both far above
// the rounding of the cap arithmetic), so a skipped pair is always farther than R.  It changes which pairs are evaluated, never a
// result: a pair's value does not depend on the other pairs, max and integer sums do not depend on order, so results are
// bit-identical whatever the launch shape.
//
// The same holds for a mode whose result does depend on order, like ScanPeak<true>'s fp64 sum, as long as one lane owns one
// (site, storm) accumulator.  A lane's sum of a storm runs over exactly the storm's records with a <= a_R, in record order: segments
// ascending, records ascending inside a segment, one lane, one accumulator.  A culled storm or segment holds none of those records
// (culling is conservative), so skipping it removes no term and moves none; padding records have NaN terms, fail a <= a_R and never
// reach the sum.  Which tile a site is in, which lane it has, which chunk the storm is in and which other storms and sites the call
// has change which segments are culled, never the terms or their order.  So the sum is bit-identical whatever the launch shape,
// the site order and the storm order.  This rests on the value being written by the one lane that accumulated it: no cross-lane or
// cross-chunk reduction may ever touch it.

namespace {

constexpr int kHzSeg = 32;                  // records per culling segment
constexpr int kHzMaxBin = 64;
constexpr double kHzPad = 1e-9;             // radians added to every cap radius
constexpr double kHzDotPad = 1e-12;         // cosine-space margin of the cap test

struct HzCap { double x, y, z, cr, sr, r, pad0, pad1; };           // cap: centre, cos / sin of radius, radius (64 bytes)

// what a prep kernel writes and the scan reads
template <class Rec>
struct ScanRows {
    Rec *rec;                               // [n_trk][n_seg_max * kHzSeg]
    HzCap *seg;                             // [n_trk][n_seg_max]
    HzCap *storm;                           // [n_trk]
    int32_t *cnt;                           // [n_trk] records
    int64_t n_seg_max;
};

// one site's terms: half angles (distance), full angles (direction); a policy's value() reads what it needs, the rest is dead code
struct ScanSite { double sp, cp, sl, cl, cosp, sinp, sinl, cosl; };

// what the scan is told that does not depend on the record type
struct ScanArgs {
    const int64_t *chunks;                  // [n_chunk][3]: storm begin, storm end, group
    const double *site_lon, *site_lat;
    int64_t n_site, n_tile, n_trk;
    double a_R, r_ang;                      // a threshold of R, R in radians
    int32_t n_cell;                         // partial counts of a (chunk, site): what the mode writes and k_hazard_reduce sums
    double thr[kHzMaxBin];                  // the call's thresholds; the mode knows which lists they are
    int32_t *part;                          // [n_chunk][n_site][n_cell]
    double *site_max;                       // [n_site][n_trk] or NULL
    unsigned long long *pairs;              // pairs evaluated (after culling)
};

// what a mode's members see of their lane
struct ScanLane {
    const ScanArgs &a;
    int32_t *lds;                           // the wave's LDS: cell k of this lane is [k * 64 + lane], in the mode's cell type
    int lane;
    int64_t tile, chunk, site, my;          // my: site, or the tile's first site for a lane without one (an index that can be read)
    bool valid;                             // the lane has a site
};

// what a mode tells the host about a call: the partial counts of a (chunk, site), the LDS bytes of a wave, the thresholds
struct ScanShape {
    int32_t n_cell;
    size_t lds;
    int32_t n_thr;
    const double *thr;
};

// Wave-uniform reads of data no kernel here writes while it runs: through the constant address space, so that the compiler issues
// scalar loads (the values then feed the fp64 VALU as SGPR operands) instead of vector loads of one address per lane.
template <typename T>
__device__ __forceinline__ T hz_uniform(const T *p) { return *(const __attribute__((address_space(4))) T *)p; }
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
// the angle (radians) of an included pair from its haversine argument, as the profile policies use it (a <= a_R < 1: no clamp)
__device__ __forceinline__ double scan_pair_angle(double a) { return 2.0 * asin(sqrt(a)); }

__device__ __forceinline__ double wave_max(double x)
{
    for (int o = 32; o >= 1; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

// the same butterfly with +: a + b == b + a bit for bit, so every lane ends with the same sum, in an order fixed by the lane numbers
__device__ __forceinline__ double wave_sum(double x)
{
    for (int o = 32; o >= 1; o >>= 1) x = x + __shfl_xor(x, o, 64);
    return x;
}

// the number of the n ascending thresholds thr that are <= m (0 for a NaN: no comparison holds): a storm's place in a histogram
__device__ __forceinline__ int scan_rank(const double *thr, int n, double m)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (thr[mid] <= m) lo = mid + 1; else hi = mid; }
    return lo;
}

constexpr int kScanMaxRow = 8;              // rows of a stacked histogram: the per-row accumulators of a mode on it

// where the rows of a stacked histogram go: launch-uniform, embedded in the policy of a mode on ScanStack (N accumulators, the
// call's n_row <= N)
template <int N>
struct ScanStackOut {
    static_assert(N >= 1 && N <= kScanMaxRow, "a stacked mode has 1 to kScanMaxRow row accumulators");
    int32_t n_row, n_hbin;
    double *plane[N];                       // [n_site][n_trk] each, or NULL
};

// The histogram tail of a mode with up to kScanMaxRow values per storm (rows: levels, windows), all ranked against the one list of
// n_hbin thresholds in thr: cells [n_row][n_hbin + 1][64] of int32, the storms of this lane whose value of the row passes exactly
// k thresholds; partial counts [row][threshold], n_cell = n_row n_hbin, which k_hazard_reduce sums unchanged.  A mode keeps its
// values in fixed arrays and calls finish under `#pragma unroll` / `if (row < n_row)`, so that they stay registers.
struct ScanStack {
    static ScanShape shape(int32_t n_row, int32_t n_hbin, size_t extra_lds_bytes, const double *thr)
    {
        return ScanShape{n_row * n_hbin, sizeof(int32_t) * 64 * (size_t)n_row * (n_hbin + 1) + extra_lds_bytes, n_hbin, thr};
    }
    static __device__ __forceinline__ void begin(const ScanLane &c, int n_row, int n_hbin)
    {
        for (int k = 0; k < n_row * (n_hbin + 1); ++k) c.lds[k * 64 + c.lane] = 0;
    }
    static __device__ __forceinline__ void count(const ScanLane &c, int row, int n_hbin, double v)
    {
        c.lds[(row * (n_hbin + 1) + scan_rank(c.a.thr, n_hbin, v)) * 64 + c.lane] += 1;
    }
    // a row of storm s: the lane that accumulated v writes it to the row's plane; with `any` (the storm has an included record)
    // it is counted
    template <int N>
    static __device__ __forceinline__ void finish(const ScanStackOut<N> &o, const ScanLane &c, int row, int64_t s, bool any, double v)
    {
        if (o.plane[row] && c.valid) o.plane[row][c.site * c.a.n_trk + s] = v;
        if (any) count(c, row, o.n_hbin, v);
    }
    static __device__ __forceinline__ void end_chunk(const ScanLane &c, int n_row, int n_hbin)    // exactly k -> at least b + 1, per row
    {
        if (!c.valid) return;
        int32_t *out = c.a.part + (c.chunk * c.a.n_site + c.site) * c.a.n_cell;
        for (int r = 0; r < n_row; ++r) {
            int32_t n = 0;
            for (int b = n_hbin - 1; b >= 0; --b) { n += c.lds[(r * (n_hbin + 1) + b + 1) * 64 + c.lane]; out[r * n_hbin + b] = n; }
        }
    }
};

// The mode of a peak: the max of value over a storm's included records, or with SUM their sum in record order (the first included
// record replaces the NaN start, every later one is added to it: nothing is ever added to a NaN), to site_max; the one-row
// ScanStack with n_hbin = n_cell.
template <bool SUM>
struct ScanPeak {
    struct Storm { double m = NAN; };
    static ScanShape shape(int32_t n_bin, const double *thr) { return ScanStack::shape(1, n_bin, 0, thr); }
    template <class P> __device__ __forceinline__ void begin(const P &, const ScanLane &c) { ScanStack::begin(c, 1, c.a.n_cell); }
    template <class P, class Rec> __device__ __forceinline__ void add(const P &pol, Storm &st, const ScanSite &me, const Rec &p, double q)
    {
        if constexpr (SUM) { const double v = pol.value(me, p, q); st.m = isnan(st.m) ? v : st.m + v; }     // in record order
        else st.m = fmax(st.m, pol.value(me, p, q));    // fmax skips NaN: the start, or a NaN value
    }
    // the two halves of end_storm, for a mode that does something between them
    __device__ __forceinline__ void store(const ScanLane &c, int64_t s, double m)
    {
        if (c.a.site_max && c.valid) c.a.site_max[c.site * c.a.n_trk + s] = m;
    }
    __device__ __forceinline__ void count(const ScanLane &c, double m)
    {
        if (!isnan(m)) ScanStack::count(c, 0, c.a.n_cell, m);
    }
    template <class P> __device__ __forceinline__ void end_storm(const P &, const ScanLane &c, const Storm &st, int64_t s, bool)
    {
        store(c, s, st.m);
        count(c, st.m);
    }
    template <class P> __device__ __forceinline__ void end_chunk(const P &, const ScanLane &c) { ScanStack::end_chunk(c, 1, c.a.n_cell); }
};

// The track of a prep kernel (one wave): the number of samples before the first j in [0, n_t) with bad(j), n_t when there is none.
template <class Bad>
__device__ __forceinline__ int64_t scan_track_len(int64_t n_t, Bad bad)
{
    const int lane = threadIdx.x;
    for (int64_t j0 = 0; j0 < n_t; j0 += 64) {
        const int64_t j = j0 + lane;
        const unsigned long long m = __ballot(j < n_t && bad(j));
        if (m) return j0 + __ffsll((long long)m) - 1;
    }
    return n_t;
}

// cap (centre = the record at `mid`, radius = the largest angle from it) of the records [b, e) of one row
template <class Rec>
__device__ void hz_cap(const Rec *row, int b, int e, HzCap *out)
{
    const int lane = threadIdx.x;
    const Rec &c = row[b + (e - b) / 2];
    double r = 0.0;
    for (int j = b + lane; j < e; j += 64) {
        const Rec &p = row[j];
        r = fmax(r, hz_angle(hz_a(c.sp, c.cp, c.sl, c.cl, c.cosp, p.sp, p.cp, p.sl, p.cl, p.cosp)));
    }
    r = wave_max(r) + kHzPad;
    if (lane == 0) {
        c.centre(out);
        out->cr = cos(r); out->sr = sin(r); out->r = r; out->pad0 = out->pad1 = 0.0;
    }
}

// the end of a prep kernel, whose lanes have written the n records of storm s to the front of its row
template <class Rec>
__device__ void scan_finish_row(const ScanRows<Rec> &o, int64_t s, int n)
{
    const int lane = threadIdx.x;
    Rec *row = o.rec + s * o.n_seg_max * kHzSeg;
    // the rest of the last segment: records no distance test passes (NaN terms), so that every segment is kHzSeg records long.
    // Written slot by slot as doubles, so a record's int64 slots hold NaN bits: no pair of a padding record is included, and no
    // mode reads a record outside add
    Rec pad;
    for (size_t i = 0; i < sizeof(Rec) / sizeof(double); ++i) reinterpret_cast<double *>(&pad)[i] = NAN;
    for (int j = n + lane; j < (n + kHzSeg - 1) / kHzSeg * kHzSeg; j += 64) row[j] = pad;
    __syncthreads();                                    // the caps read records other lanes wrote
    if (lane == 0) o.cnt[s] = n;
    if (n == 0) return;
    hz_cap(row, 0, n, o.storm + s);
    for (int k = 0; k * kHzSeg < n; ++k) hz_cap(row, k * kHzSeg, min(n, (k + 1) * kHzSeg), o.seg + s * o.n_seg_max + k);
}

// true when no point of the cap can be within the tile's padded radius (cos_t, sin_t, r_t) of the tile centre (tx, ty, tz)
__device__ __forceinline__ bool hz_far(const HzCap &c, double tx, double ty, double tz, double ct, double st, double rt)
{
    if (c.r + rt >= kPi) return false;
    const double dot = c.x * tx + c.y * ty + c.z * tz;
    return dot < c.cr * ct - c.sr * st - kHzDotPad;     // angle(centres) > r_cap + r_tile
}

template <class Policy>
__global__ __launch_bounds__(64) void k_site_scan(ScanArgs a, ScanRows<typename Policy::Rec> rows, Policy pol)
{
    using Rec = typename Policy::Rec;
    using Mode = typename Policy::Mode;
    extern __shared__ int32_t scan_lds[];
    const int lane = threadIdx.x;
    const int64_t tile = blockIdx.x % a.n_tile, chunk = blockIdx.x / a.n_tile;
    const int64_t site = tile * 64 + lane;
    const bool valid = site < a.n_site;
    const int64_t site0 = tile * 64;
    const int64_t my = valid ? site : site0;
    const double y = a.site_lat[my], x = a.site_lon[my];
    const double hp = y * (kPi / 360.0), hl = x * (kPi / 360.0), phi = y * (kPi / 180.0), lam = x * (kPi / 180.0);
    const ScanSite me{sin(hp), cos(hp), sin(hl), cos(hl), cos(phi), sin(phi), sin(lam), cos(lam)};
    const ScanLane c{a, scan_lds, lane, tile, chunk, site, my, valid};
    Mode mode;
    mode.begin(pol, c);

    // tile cap: centre = the tile's first site, radius = the largest angle from it, padded by R
    const double sp0 = __shfl(me.sp, 0, 64), cp0 = __shfl(me.cp, 0, 64), sl0 = __shfl(me.sl, 0, 64), cl0 = __shfl(me.cl, 0, 64);
    const double cosp0 = __shfl(me.cosp, 0, 64);
    const double rt = wave_max(hz_angle(hz_a(sp0, cp0, sl0, cl0, cosp0, me.sp, me.cp, me.sl, me.cl, me.cosp))) + kHzPad + a.r_ang + kHzPad;
    const double phi0 = __shfl(y, 0, 64) * (kPi / 180.0), lam0 = __shfl(x, 0, 64) * (kPi / 180.0);
    const double tx = cos(phi0) * cos(lam0), ty = cos(phi0) * sin(lam0), tz = sin(phi0);
    const double ct = cos(rt), st = sin(rt);

    const int64_t s_begin = hz_uniform(a.chunks + 3 * chunk), s_end = hz_uniform(a.chunks + 3 * chunk + 1);
    const unsigned long long n_lanes = (unsigned long long)min<int64_t>(64, a.n_site - site0);
    unsigned long long pairs = 0;
    __syncthreads();
    for (int64_t s = s_begin; s < s_end; ++s) {
        typename Mode::Storm acc;
        bool near = false;                              // the storm's cap reaches the tile (wave-uniform)
        const int n = hz_uniform(rows.cnt + s);
        if (n > 0 && !hz_far(hz_uniform(rows.storm + s), tx, ty, tz, ct, st, rt)) {
            near = true;
            const Rec *row = rows.rec + s * rows.n_seg_max * kHzSeg;
            const HzCap *segs = rows.seg + s * rows.n_seg_max;
            for (int k = 0; k * kHzSeg < n; ++k) {
                if (hz_far(hz_uniform(segs + k), tx, ty, tz, ct, st, rt)) continue;
                pairs += (unsigned long long)(min(n, (k + 1) * kHzSeg) - k * kHzSeg);
                const Rec *seg = row + k * kHzSeg;
#pragma unroll Policy::kUnroll
                for (int j = 0; j < kHzSeg; ++j) {                  // (padding records fail the test: NaN terms)
                    const Rec p = Rec::uniform(seg + j);
                    const double q = hz_a(me.sp, me.cp, me.sl, me.cl, me.cosp, p.sp, p.cp, p.sl, p.cl, p.cosp);
                    if (q <= a.a_R) mode.add(pol, acc, me, p, q);
                }
            }
        }
        mode.end_storm(pol, c, acc, s, near);
    }
    mode.end_chunk(pol, c);
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

// ---------------------------------------------------------------------------------------------------------------- host

// the arguments every analysis has; `who` is the entry point's prefix ("tcr_hazard"), n_t_rule its bound on n_t in words
template <class Tracks>
int scan_check(tcr_ctx *ctx, const char *who, const Tracks *t, int64_t n_t_max, const char *n_t_rule, int64_t n_site, int32_t n_bin,
               const double *thr)
{
    if (n_bin < 1 || n_bin > kHzMaxBin) return fail(ctx, "%s: n_bin must be in [1, 64]", who);
    for (int b = 0; b < n_bin; ++b)
        if (!std::isfinite(thr[b]) || (b > 0 && !(thr[b] > thr[b - 1]))) return fail(ctx, "%s: thresholds must be finite and ascending", who);
    if (n_site < 1 || t->n_trk < 0 || t->n_t < 1 || t->n_t > n_t_max || t->row_stride < t->n_t || t->n_group < 1)
        return fail(ctx, "%s: bad sizes (n_site >= 1, %s, row_stride >= n_t, n_group >= 1)", who, n_t_rule);
    if (t->group_off[0] != 0 || t->group_off[t->n_group] != t->n_trk) return fail(ctx, "%s: group_off must run from 0 to n_trk", who);
    for (int32_t g = 0; g < t->n_group; ++g)
        if (t->group_off[g + 1] < t->group_off[g]) return fail(ctx, "%s: group_off must not decrease", who);
    return 0;
}

// the rows of a call on ScanStack; row: their name in the entry point's arguments ("level": n_level)
inline int scan_stack_check(tcr_ctx *ctx, const char *who, const char *row, int32_t n_row, int32_t n_bin)
{
    if (n_row < 1 || n_row > kScanMaxRow) return fail(ctx, "%s: n_%s must be in [1, 8]", who, row);
    if ((int64_t)n_row * ((int64_t)n_bin + 1) > kHzMaxBin) return fail(ctx, "%s: n_%s * (n_bin + 1) must be <= 64", who, row);
    return 0;
}

// The launch shape of one call: tiles of 64 sites, and every group split into chunks of at most `ch` storms, sized so that the
// grid has ~8192 waves.  tab: [n_chunk][3] storm begin, storm end, group; gch: [n_group + 1] the first chunk of every group.  A
// function of the group offsets, n_site and max_chunk (the most storms a chunk may hold) alone.  An analysis makes it once per call
// and sizes its own per-chunk workspaces from it; on the device the two tables lie one after the other (scan_dev_tab).
struct ScanPlan {
    int64_t n_tile, n_chunk;
    std::vector<int64_t> tab, gch;
};
constexpr int64_t kScanAnyChunk = INT64_MAX;            // max_chunk of a mode that can count any number of storms

template <class Tracks>
ScanPlan scan_plan(const Tracks *t, int64_t n_site, int64_t max_chunk)
{
    ScanPlan p;
    p.n_tile = (n_site + 63) / 64;
    const int64_t want = std::max<int64_t>(1, (8192 + p.n_tile - 1) / p.n_tile);
    const int64_t ch = std::min(max_chunk, std::max<int64_t>(16, (t->n_trk + want - 1) / want));
    p.gch.assign(1, 0);
    for (int64_t g = 0; g < t->n_group; ++g) {
        for (int64_t b = t->group_off[g]; b < t->group_off[g + 1]; b += ch) {
            p.tab.push_back(b); p.tab.push_back(std::min(b + ch, (int64_t)t->group_off[g + 1])); p.tab.push_back(g);
        }
        p.gch.push_back((int64_t)p.tab.size() / 3);
    }
    p.n_chunk = (int64_t)p.tab.size() / 3;
    return p;
}

// the plan's tables on the device once scan_run has enqueued their upload: tab, then (at + plan.tab.size()) gch
inline const int64_t *scan_dev_tab(const ScanWs &w) { return reinterpret_cast<const int64_t *>(w.d[kWsTab].p); }

// the haversine argument sin^2(angle / 2) of radius_km on a sphere of re_km: what a pair's a is tested against
inline double scan_a_of(double radius_km, double re_km)
{
    const double h = sin(radius_km / (2.0 * re_km));
    return h * h;
}

// what scan_run hands the launch step next to the rows: the scan's arguments, grid, LDS bytes and stream
struct ScanLaunch {
    ScanArgs args;
    dim3 grid;
    size_t lds;
    hipStream_t st;
};

// One call on stream st: workspaces, the plan's tables, launch, reduction.  launch(rows, ScanLaunch, the prep kernel's workspace)
// enqueues the analysis's prep kernel, then its k_site_scan instantiation (scan_launch), and returns the first launch error.
// shape: of the policy's mode; n_rec: the most records a storm can have; radius_km on a sphere of re_km (where a policy has two
// radii, the larger); extra_bytes: what the prep kernel wants in its workspace.
template <class Rec, class Tracks, class Launch>
int scan_run(tcr_ctx *ctx, ScanWs &w, const char *who, const Tracks *t, const ScanPlan &plan, const ScanShape &shape, int64_t n_rec,
             size_t extra_bytes, int64_t n_site, const double *site_lon, const double *site_lat, double radius_km, double re_km,
             int32_t *counts, double *site_max, hipStream_t st, Launch launch)
{
    const int64_t n_trk = t->n_trk, n_group = t->n_group, n_tile = plan.n_tile, n_chunk = plan.n_chunk;
    const int64_t n_seg_max = (n_rec + kHzSeg - 1) / kHzSeg;
    const int32_t n_cell = shape.n_cell;
    if (n_tile * n_chunk >= ((int64_t)1 << 31) || n_site * n_group * n_cell >= ((int64_t)1 << 39))
        return fail(ctx, "%s: too many sites x storm chunks for one launch; split the sites", who);
    const size_t n_tab = plan.tab.size() + plan.gch.size();

    if (w.d[kWsRec].grow(ctx, sizeof(Rec) * (size_t)std::max<int64_t>(1, n_trk * n_seg_max * kHzSeg)) < 0 ||
        w.d[kWsCaps].grow(ctx, sizeof(HzCap) * (size_t)std::max<int64_t>(1, n_trk * (n_seg_max + 1))) < 0 ||
        w.d[kWsCnt].grow(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(1, n_trk)) < 0 ||
        w.d[kWsPart].grow(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(1, n_chunk * n_site * n_cell)) < 0 ||
        w.d[kWsTab].grow(ctx, sizeof(int64_t) * (n_tab + 1)) < 0 ||
        (extra_bytes && w.d[kWsPrep].grow(ctx, extra_bytes) < 0))
        return -1;
    // the tables go up through a pinned buffer of the workspace; the previous call's upload must be done with it
    if (w.ev) HIPCHK(ctx, hipEventSynchronize(w.ev));
    else {
        HIPCHK(ctx, hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    }
    if (w.h.cap < n_tab) HIPCHK(ctx, w.h.alloc(n_tab));
    memcpy(w.h.p, plan.tab.data(), plan.tab.size() * sizeof(int64_t));
    memcpy(w.h.p + plan.tab.size(), plan.gch.data(), plan.gch.size() * sizeof(int64_t));
    int64_t *d_tab = reinterpret_cast<int64_t *>(w.d[kWsTab].p);
    unsigned long long *d_pairs = reinterpret_cast<unsigned long long *>(d_tab + n_tab);
    HIPCHK(ctx, hipMemcpyAsync(d_tab, w.h.p, n_tab * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(w.ev, st));
    HIPCHK(ctx, hipMemsetAsync(d_pairs, 0, sizeof(unsigned long long), st));
    w.pairs = d_pairs;

    HzCap *caps = reinterpret_cast<HzCap *>(w.d[kWsCaps].p);
    int32_t *part = reinterpret_cast<int32_t *>(w.d[kWsPart].p);
    if (n_trk > 0) {                                    // (then every storm is in a chunk: n_chunk > 0)
        const ScanRows<Rec> rows{reinterpret_cast<Rec *>(w.d[kWsRec].p), caps + n_trk, caps, reinterpret_cast<int32_t *>(w.d[kWsCnt].p),
                                 n_seg_max};
        ScanLaunch L{};
        ScanArgs &m = L.args;
        m.chunks = d_tab;
        m.site_lon = site_lon; m.site_lat = site_lat;
        m.n_site = n_site; m.n_tile = n_tile; m.n_trk = n_trk;
        m.a_R = scan_a_of(radius_km, re_km); m.r_ang = radius_km / re_km;
        m.n_cell = n_cell;
        for (int b = 0; b < shape.n_thr; ++b) m.thr[b] = shape.thr[b];
        m.part = part; m.site_max = site_max; m.pairs = d_pairs;
        L.grid = dim3((unsigned)(n_tile * n_chunk)); L.lds = shape.lds; L.st = st;
        HIPCHK(ctx, launch(rows, L, w.d[kWsPrep].p));
    }
    const int64_t n_out = n_site * n_group * n_cell;
    hipLaunchKernelGGL(k_hazard_reduce, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, part, d_tab + plan.tab.size(), n_site,
                       (int32_t)n_group, n_cell, counts);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(w.done, st));
    return 0;
}

// What a launch step enqueues: the analysis's prep kernel (one block of 64 lanes per storm) on p, then Policy's scan of the rows.
template <class Policy, class PrepArgs>
hipError_t scan_launch(void (*prep)(PrepArgs), const PrepArgs &p, const ScanRows<typename Policy::Rec> &rows, const ScanLaunch &L,
                       const Policy &pol)
{
    hipLaunchKernelGGL(prep, dim3((unsigned)L.args.n_trk), dim3(64), 0, L.st, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_site_scan<Policy>, L.grid, dim3(64), L.lds, L.st, L.args, rows, pol);
    return hipGetLastError();
}

// the sites and outputs of a _host entry point on the device (buffers of B), and the way back
struct ScanHostIO {
    const double *site_lon, *site_lat;
    int32_t *counts;
    double *site_max;
    size_t n_out, n_max, n_plane;           // n_max: values of a [n_site][n_trk] plane; n_plane: what is allocated for one (>= 1)
    bool ok;
};

template <class Tracks>
ScanHostIO scan_host_io(DevBuf &B, const Tracks *t, int64_t n_site, const double *site_lon, const double *site_lat, int32_t n_cell,
                        bool want_max)
{
    ScanHostIO d{};
    d.site_lon = B.put(site_lon, (size_t)n_site); d.site_lat = B.put(site_lat, (size_t)n_site);
    d.n_out = (size_t)n_site * t->n_group * n_cell; d.n_max = (size_t)n_site * t->n_trk;
    d.n_plane = (size_t)n_site * std::max<int64_t>(1, t->n_trk);
    d.counts = B.get<int32_t>(d.n_out);
    d.site_max = want_max ? B.get<double>(d.n_plane) : nullptr;
    d.ok = d.site_lon && d.site_lat && d.counts && (!want_max || d.site_max);
    return d;
}

// The further optional [n_site][n_trk] planes of a _host entry point, host[0 .. n) (host itself may be NULL): dev[i] is a plane of
// B for every host[i] that is not NULL, else NULL.  false: an allocation failed.
inline bool scan_host_planes(DevBuf &B, const ScanHostIO &d, int n, double *const *host, double **dev)
{
    for (int i = 0; i < n; ++i) {
        dev[i] = nullptr;
        if (host && host[i] && !(dev[i] = B.get<double>(d.n_plane))) return false;
    }
    return true;
}

// their way back, enqueued on the context's stream: before scan_download, which waits for it
inline int scan_download_planes(tcr_ctx *ctx, const ScanHostIO &d, int n, double *const *host, double *const *dev)
{
    for (int i = 0; i < n; ++i)
        if (dev[i] && d.n_max) HIPCHK(ctx, hipMemcpyAsync(host[i], dev[i], sizeof(double) * d.n_max, hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

int scan_download(tcr_ctx *ctx, const ScanHostIO &d, int32_t *counts, double *site_max)
{
    HIPCHK(ctx, hipMemcpyAsync(counts, d.counts, sizeof(int32_t) * d.n_out, hipMemcpyDeviceToHost, ctx->stream));
    if (site_max) HIPCHK(ctx, hipMemcpyAsync(site_max, d.site_max, sizeof(double) * d.n_max, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// pairs the last call on w evaluated; `who` as in scan_check
int scan_pairs(tcr_ctx *ctx, const ScanWs &w, const char *who, int64_t *pairs)
{
    if (!pairs) return fail(ctx, "%s_pairs: NULL argument", who);
    if (!w.pairs) return fail(ctx, "%s_pairs: no %s_* call on this context yet", who, who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned long long v = 0;
    HIPCHK(ctx, hipEventSynchronize(w.done));
    HIPCHK(ctx, copy_sync(ctx->stream, &v, w.pairs, sizeof v, hipMemcpyDeviceToHost));
    *pairs = (int64_t)v;
    return 0;
}

}  // namespace
