// The site scan: what the per-site analyses of a track ensemble (tcr_hazard.hip, tcr_windfield.hip, tcr_loss.hip, tcr_rainfall.hip,
// tcr_compound.hip, tcr_duration.hip) share.  Each of them turns
// every storm into a row of wave-uniform records, and wants
//
//   site_max[site][storm] = max of value(site, record) over the storm's records with haversine(site, record) <= R   (NaN: none)
//   counts[site][group][bin] = #storms of the group with site_max >= thr[bin]
//
// An analysis supplies
//   a record type   plain doubles that begin with the half-angle terms { sp, cp, sl, cl, cosp } of the point (the distance test),
//                   with  static Rec uniform(const Rec *)  (the terms a pair reads, through scalar loads)  and
//                   void centre(HzCap *) const  (the unit vector of the point, for a cap centred on it);
//   a prep kernel   one wave per storm: writes the storm's records to the front of its row and ends with scan_finish_row
//                   (NaN padding of the last segment, record count, bounding caps of the storm and of every kHzSeg-record segment);
//   a policy        { Rec, kUnroll, value(site, record, a) }: a compile-time type that travels to the kernel by value, so that it
//                   can carry launch-uniform parameters.  Nothing here branches at run time on which analysis is running.
//                   A policy with `static constexpr bool kLoss = true` (tcr_loss.hip) turns on the loss variant of the scan at
//                   compile time: site_terms(site, valid) -> per-lane terms, loss(terms, m) -> the lane's loss of a storm, and
//                   the buffers tile_loss [n_tile][n_trk] and site_part [n_chunk][n_site].  Per storm the wave sums its 64 lane
//                   losses with a fixed butterfly and lane 0 stores the sum; every lane keeps a running sum of its own losses in
//                   storm order.  Policies without kLoss compile to the code they had before the variant existed.
//                   A policy with `static constexpr bool kSum = true` (tcr_rainfall.hip) turns max into a sum at compile time:
//                   site_max[site][storm] = sum of value(site, record) over the same records, in record order (NaN: none).  The
//                   first included record replaces the NaN start, every later one is added to it: nothing is ever added to a NaN.
//                   kSum with kLoss is a static_assert.  Policies without kSum compile to the code they had before it existed.
//                   A policy with `static constexpr bool kJoint = true` (tcr_compound.hip) scans two hazards of one record at
//                   once: the pair's angle is formed once, first(site, record, angle) goes into a max under the policy's a_first and
//                   second(site, record, angle) into a max, or with kSecondSum into a sum in record order, under its a_second;
//                   a_R and r_ang (the culling) are those of the larger radius.  site_max takes the first, the policy's
//                   site_second the second.  thr holds the n_first thresholds of the first, then the n_second of the second, and
//                   the histogram is two-dimensional: n_bin = (n_first + 1) (n_second + 1) and
//                   counts[site][group][a (n_second + 1) + b] = #storms of the group passing at least a thresholds of the first and
//                   at least b of the second (a NaN passes none, so index 0 is "no condition" and [0][0] the size of the group).
//                   A wave's histogram is its LDS, and 64 cells of int32 per lane (16 KB) leave room for 9 waves on a CU: the
//                   joint scan ran at 2 waves / SIMD and 1.6 x slower than with 9 cells (profiles/compound_bench.txt).  So the
//                   joint histogram's cells are kJointHist (16 bits), and the caller keeps a chunk at kJointMaxChunk storms or
//                   fewer (scan_run's max_chunk), which no cell and no suffix sum can exceed.
//                   kJoint with kLoss or kSum is a static_assert.  Policies without kJoint compile to the code they had before it.
//                   A policy with `static constexpr int kLevels = N` (1 <= N <= kScanMaxLevel; tcr_duration.hip) measures time
//                   instead of a peak: value(site, record, a) is formed once per included pair and compared with the policy's N
//                   ascending level[] (unused ones +inf), and the record's integer weight(record) is added to the int32
//                   accumulator of every level the value reaches (>=) and to one more that counts the included records.  The N + 1
//                   accumulators are registers: fixed arrays, fully unrolled, never indexed by a run-time value.  Per storm each
//                   of the policy's n_level levels has the value (double)sum * unit (NaN when no record was included), which the
//                   lane that accumulated it writes to the policy's site_level[l] (when not NULL) and ranks against the n_hbin
//                   thresholds in thr into the level's own (n_hbin + 1) cells of the histogram, which therefore has
//                   n_level (n_hbin + 1) cells: the caller passes n_bin = n_level n_hbin (the partial counts it gets,
//                   [level][threshold], which k_hazard_reduce sums unchanged) and launches with LDS for those cells instead of the
//                   bytes it is handed.  Every lane also keeps an int64 total of its sums per level over the chunk's storms and
//                   writes it to the policy's level_part [n_chunk][n_site][n_level].  There is no max: the caller passes site_max = NULL.
//                   kLevels with kLoss, kSum or kJoint is a static_assert.  Policies without kLevels compile to the code they had
//                   before it existed.
// and calls scan_run with a workspace of its own (ScanWs, six instances in tcr_ctx: a hazard, a footprint, a loss, a rainfall, a
// compound and a duration call may be in flight on different streams of one context).
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
// The same holds for a kSum policy, although an fp64 sum does depend on its order.  A lane's sum of a storm runs over exactly the
// storm's records with a <= a_R, in record order: segments ascending, records ascending inside a segment, one lane, one accumulator.
// A culled storm or segment holds none of those records (culling is conservative), so skipping it removes no term and moves none;
// padding records have NaN terms, fail a <= a_R and never reach the sum.  Which tile a site is in, which lane it has, which chunk
// the storm is in and which other storms and sites the call has change which segments are culled, never the terms or their order.
// So the sum is bit-identical whatever the launch shape, the site order and the storm order.  This rests on site_max being written
// by the one lane that accumulated it: no cross-lane or cross-chunk reduction may ever touch it.
//
// And for a kJoint policy.  Each of its two accumulators sees exactly the records with a <= its own a threshold, in record order,
// and nothing else: the cull uses the larger radius, so it is conservative for both; the test of one hazard never gates the other;
// the values come from the functions the single-hazard policies call, on the same record terms and the same angle expression.  So
// each plane is bit for bit what the single-hazard scan of that policy writes, and the 2-D counts are integer sums of per-storm
// ranks of those values: bit-identical whatever the launch shape, the site order and the storm order.
//
// And for a kLevels policy, by the first argument alone: everything it accumulates is an integer.  A pair's value and weight do not
// depend on the other pairs, a skipped pair is never an included one, and int32 and int64 sums do not depend on order; the value
// written is one conversion and one multiply of such a sum.

namespace {

constexpr int kHzSeg = 32;                  // records per culling segment
constexpr int kHzMaxBin = 64;
constexpr int kScanMaxLevel = 8;            // levels of a kLevels policy
using kJointHist = uint16_t;                // a cell of the joint scan's LDS histogram
constexpr int64_t kJointMaxChunk = 65535;   // storms of a chunk it can count
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

template <class Rec>
struct ScanArgs {
    ScanRows<Rec> rows;
    const int64_t *chunks;                  // [n_chunk][3]: storm begin, storm end, group
    const double *site_lon, *site_lat;
    int64_t n_site, n_tile, n_trk;
    double a_R, r_ang;                      // a threshold of R, R in radians
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

// Policy::kLoss when the policy has one, false otherwise
template <class P, class = void>
struct scan_has_loss : std::false_type {};
template <class P>
struct scan_has_loss<P, std::void_t<decltype(P::kLoss)>> : std::bool_constant<P::kLoss> {};

// Policy::kSum when the policy has one, false otherwise
template <class P, class = void>
struct scan_has_sum : std::false_type {};
template <class P>
struct scan_has_sum<P, std::void_t<decltype(P::kSum)>> : std::bool_constant<P::kSum> {};

// Policy::kJoint when the policy has one, false otherwise
template <class P, class = void>
struct scan_has_joint : std::false_type {};
template <class P>
struct scan_has_joint<P, std::void_t<decltype(P::kJoint)>> : std::bool_constant<P::kJoint> {};

// Policy::kLevels (the number of level accumulators) when the policy has one, 0 otherwise
template <class P, class = void>
struct scan_levels : std::integral_constant<int, 0> {};
template <class P>
struct scan_levels<P, std::void_t<decltype(P::kLevels)>> : std::integral_constant<int, P::kLevels> {};

// the number of the n ascending thresholds thr that are <= m (0 for a NaN: no comparison holds): the joint scan's two ranks
__device__ __forceinline__ int scan_rank(const double *thr, int n, double m)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (thr[mid] <= m) lo = mid + 1; else hi = mid; }
    return lo;
}

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
    // the rest of the last segment: records no distance test passes (NaN terms), so that every segment is kHzSeg records long
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
__global__ __launch_bounds__(64) void k_site_scan(ScanArgs<typename Policy::Rec> a, Policy pol)
{
    using Rec = typename Policy::Rec;
    // [n_bin + 1][64]: storms of this lane whose max passes exactly k thresholds (kJoint: [n_first + 1][n_second + 1][64] cells of
    // kJointHist, exactly (kw, kr) of each list)
    using Hist = std::conditional_t<scan_has_joint<Policy>::value, kJointHist, int32_t>;
    extern __shared__ int32_t hist_lds[];
    Hist *hist = reinterpret_cast<Hist *>(hist_lds);
    const int lane = threadIdx.x;
    const int64_t tile = blockIdx.x % a.n_tile, chunk = blockIdx.x / a.n_tile;
    const int64_t site = tile * 64 + lane;
    const bool valid = site < a.n_site;
    const int64_t site0 = tile * 64;
    const int64_t my = valid ? site : site0;
    const double y = a.site_lat[my], x = a.site_lon[my];
    const double hp = y * (kPi / 360.0), hl = x * (kPi / 360.0), phi = y * (kPi / 180.0), lam = x * (kPi / 180.0);
    const ScanSite me{sin(hp), cos(hp), sin(hl), cos(hl), cos(phi), sin(phi), sin(lam), cos(lam)};
    constexpr int kLevels = scan_levels<Policy>::value;
    static_assert(kLevels >= 0 && kLevels <= kScanMaxLevel, "a kLevels policy has 1 to kScanMaxLevel level accumulators");
    if constexpr (kLevels > 0) {                        // kLevels: [n_level][n_hbin + 1][64]
        for (int k = 0; k < pol.n_level * (pol.n_hbin + 1); ++k) hist[k * 64 + lane] = 0;
    } else {
        for (int k = 0; k <= a.n_bin; ++k) hist[k * 64 + lane] = 0;
    }

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
    constexpr bool kLoss = scan_has_loss<Policy>::value;
    constexpr bool kSum = scan_has_sum<Policy>::value;
    static_assert(!(kSum && kLoss), "the loss variant of the scan is defined on a max");
    constexpr bool kJoint = scan_has_joint<Policy>::value;
    static_assert(!(kJoint && (kLoss || kSum)), "the joint scan has accumulators of its own: neither the loss nor the sum variant");
    static_assert(!(kLevels > 0 && (kLoss || kSum || kJoint)), "the level scan accumulates weights, not values: no other variant");
    constexpr int kNL = kLevels > 0 ? kLevels : 1;
    [[maybe_unused]] int64_t lv_total[kNL] = {};        // kLevels: this site's sums of the chunk's storms, per level
    [[maybe_unused]] double loss_acc = 0.0;             // kLoss: this site's losses of the chunk's storms, summed in storm order
    [[maybe_unused]] auto terms = [&] { if constexpr (kLoss) return pol.site_terms(my, valid); else return 0; }();
    __syncthreads();
    for (int64_t s = s_begin; s < s_end; ++s) {
        double m = NAN;
        [[maybe_unused]] double m2 = NAN;               // kJoint: the second hazard
        [[maybe_unused]] bool near = false;             // kLoss: the storm's cap reaches the tile (wave-uniform)
        [[maybe_unused]] int32_t lv[kNL] = {};          // kLevels: the weights of the records that reach each level,
        [[maybe_unused]] int32_t lv_in = 0;             // and of every included record
        const int n = hz_uniform(a.rows.cnt + s);
        if (n > 0 && !hz_far(hz_uniform(a.rows.storm + s), tx, ty, tz, ct, st, rt)) {
            if constexpr (kLoss) near = true;
            const Rec *row = a.rows.rec + s * a.rows.n_seg_max * kHzSeg;
            const HzCap *segs = a.rows.seg + s * a.rows.n_seg_max;
            for (int k = 0; k * kHzSeg < n; ++k) {
                if (hz_far(hz_uniform(segs + k), tx, ty, tz, ct, st, rt)) continue;
                pairs += (unsigned long long)(min(n, (k + 1) * kHzSeg) - k * kHzSeg);
                const Rec *seg = row + k * kHzSeg;
#pragma unroll Policy::kUnroll
                for (int j = 0; j < kHzSeg; ++j) {                  // (padding records fail the test: NaN terms)
                    const Rec p = Rec::uniform(seg + j);
                    const double q = hz_a(me.sp, me.cp, me.sl, me.cl, me.cosp, p.sp, p.cp, p.sl, p.cl, p.cosp);
                    if constexpr (kJoint) {
                        if (q <= a.a_R) {                           // the larger radius; then each hazard under its own
                            const double ang = scan_pair_angle(q);
                            if (q <= pol.a_first) m = fmax(m, pol.first(me, p, ang));
                            if (q <= pol.a_second) {
                                const double v = pol.second(me, p, ang);
                                if constexpr (Policy::kSecondSum) m2 = isnan(m2) ? v : m2 + v;          // in record order
                                else m2 = fmax(m2, v);
                            }
                        }
                    } else if constexpr (kLevels > 0) {
                        if (q <= a.a_R) {
                            const double v = pol.value(me, p, q);
                            const int32_t h = pol.weight(p);
                            lv_in += h;
#pragma unroll
                            for (int l = 0; l < kNL; ++l) lv[l] += v >= pol.level[l] ? h : 0;         // (a NaN reaches none)
                        }
                    } else if constexpr (kSum) {
                        if (q <= a.a_R) { const double v = pol.value(me, p, q); m = isnan(m) ? v : m + v; }   // in record order
                    } else {
                        if (q <= a.a_R) m = fmax(m, pol.value(me, p, q));   // fmax skips NaN: the start, or a NaN value
                    }
                }
            }
        }
        if (a.site_max && valid) a.site_max[site * a.n_trk + s] = m;
        if constexpr (kJoint) {
            if (pol.site_second && valid) pol.site_second[site * a.n_trk + s] = m2;
        }
        if constexpr (kLoss) {
            double t = 0.0;                             // a storm culled for the whole tile: 0, without the butterfly
            if (near) {
                const double l = pol.loss(terms, m);
                loss_acc += l;
                t = wave_sum(l);
            }
            if (lane == 0) pol.tile_loss[tile * a.n_trk + s] = t;
        }
        if constexpr (kLevels > 0) {                    // a plane and a rank per level; a storm without an included record counts nowhere
#pragma unroll
            for (int l = 0; l < kNL; ++l) {
                if (l < pol.n_level) {                  // (wave-uniform)
                    const double d = lv_in ? (double)lv[l] * pol.unit : NAN;
                    if (pol.site_level[l] && valid) pol.site_level[l][site * a.n_trk + s] = d;
                    if (lv_in) hist[(l * (pol.n_hbin + 1) + scan_rank(a.thr, pol.n_hbin, d)) * 64 + lane] += 1;
                    lv_total[l] += lv[l];
                }
            }
        } else if constexpr (kJoint) {                  // every storm is counted: a NaN has rank 0
            const int kw = scan_rank(a.thr, pol.n_first, m), kr = scan_rank(a.thr + pol.n_first, pol.n_second, m2);
            hist[(kw * (pol.n_second + 1) + kr) * 64 + lane] += 1;
        } else if (!isnan(m)) {
            int lo = 0, hi = a.n_bin;                   // k = #thresholds <= m
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.thr[mid] <= m) lo = mid + 1; else hi = mid; }
            hist[lo * 64 + lane] += 1;
        }
    }
    if constexpr (kJoint) {
        // exactly (kw, kr) -> at least (kw, kr): suffix sums along the second axis, then along the first, in the lane's own column
        const int nw = pol.n_first, nr = pol.n_second;
        for (int kw = nw; kw >= 0; --kw)
            for (int kr = nr - 1; kr >= 0; --kr) hist[(kw * (nr + 1) + kr) * 64 + lane] += hist[(kw * (nr + 1) + kr + 1) * 64 + lane];
        for (int kw = nw - 1; kw >= 0; --kw)
            for (int kr = nr; kr >= 0; --kr) hist[(kw * (nr + 1) + kr) * 64 + lane] += hist[((kw + 1) * (nr + 1) + kr) * 64 + lane];
    }
    if (valid) {
        [[maybe_unused]] int32_t c = 0;
        int32_t *out = a.part + (chunk * a.n_site + site) * a.n_bin;
        if constexpr (kLevels > 0) {                    // at least b + 1 thresholds, per level; and the level's total
            for (int l = 0; l < pol.n_level; ++l) {
                int32_t cl = 0;
                for (int b = pol.n_hbin - 1; b >= 0; --b) { cl += hist[(l * (pol.n_hbin + 1) + b + 1) * 64 + lane]; out[l * pol.n_hbin + b] = cl; }
            }
#pragma unroll
            for (int l = 0; l < kNL; ++l)
                if (l < pol.n_level) pol.level_part[(chunk * a.n_site + site) * pol.n_level + l] = lv_total[l];
        } else if constexpr (kJoint) {
            for (int b = 0; b < a.n_bin; ++b) out[b] = hist[b * 64 + lane];
        } else {
            for (int b = a.n_bin - 1; b >= 0; --b) { c += hist[(b + 1) * 64 + lane]; out[b] = c; }
        }
        if constexpr (kLoss) pol.site_part[chunk * a.n_site + site] = loss_acc;
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

// ---------------------------------------------------------------------------------------------------------------- host
// ScanWs::d (blocks in bytes): 0 records, 1 caps (storms, then segments), 2 record counts, 3 partial counts, 4 chunk table + pair
// counter, 5 the prep kernel's own workspace, 6 and 7 the analysis's own (tcr_loss.hip: tile losses, per-chunk site losses;
// tcr_duration.hip: 6 the per-chunk level totals)

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

// chunks: every group split into pieces of at most `ch` storms, sized so that the grid has ~8192 waves.  tab: [n_chunk][3] storm
// begin, storm end, group; gch: [n_group + 1] the first chunk of every group.  A function of the group offsets and n_tile alone,
// and of max_chunk, the most storms a chunk may hold.
template <class Tracks>
void scan_chunks(const Tracks *t, int64_t n_tile, std::vector<int64_t> &tab, std::vector<int64_t> &gch, int64_t max_chunk = INT64_MAX)
{
    const int64_t want = std::max<int64_t>(1, (8192 + n_tile - 1) / n_tile);
    const int64_t ch = std::min(max_chunk, std::max<int64_t>(16, (t->n_trk + want - 1) / want));
    tab.clear(); gch.assign(1, 0);
    for (int64_t g = 0; g < t->n_group; ++g) {
        for (int64_t b = t->group_off[g]; b < t->group_off[g + 1]; b += ch) {
            tab.push_back(b); tab.push_back(std::min(b + ch, (int64_t)t->group_off[g + 1])); tab.push_back(g);
        }
        gch.push_back((int64_t)tab.size() / 3);
    }
}

// the haversine argument sin^2(angle / 2) of radius_km on a sphere of re_km: what a pair's a is tested against
inline double scan_a_of(double radius_km, double re_km)
{
    const double h = sin(radius_km / (2.0 * re_km));
    return h * h;
}

// One call on stream st: chunk table, workspaces, launch, reduction.  launch(args, workspace 5, grid, LDS bytes) enqueues the
// analysis's prep kernel, then its k_site_scan instantiation, and returns the first launch error.  n_rec: the most records a
// storm can have; radius_km on a sphere of re_km; extra_bytes: what the prep kernel wants in workspace 5.  A kJoint policy's call
// passes n_bin = (n_first + 1) (n_second + 1), kHzMaxBin thresholds (its two lists, then anything), the larger radius and
// max_chunk = kJointMaxChunk, and launches with LDS for kJointHist cells instead of the int32 bytes it is handed.
template <class Rec, class Tracks, class Launch>
int scan_run(tcr_ctx *ctx, ScanWs &w, const char *who, const Tracks *t, int64_t n_rec, size_t extra_bytes, int64_t n_site,
             const double *site_lon, const double *site_lat, double radius_km, double re_km, int32_t n_bin, const double *thresholds,
             int32_t *counts, double *site_max, hipStream_t st, Launch launch, int64_t max_chunk = INT64_MAX)
{
    const int64_t n_trk = t->n_trk, n_group = t->n_group;
    const int64_t n_tile = (n_site + 63) / 64, n_seg_max = (n_rec + kHzSeg - 1) / kHzSeg;

    std::vector<int64_t> tab, gch;
    scan_chunks(t, n_tile, tab, gch, max_chunk);
    const int64_t n_chunk = (int64_t)tab.size() / 3;
    if (n_tile * n_chunk >= ((int64_t)1 << 31) || n_site * n_group * n_bin >= ((int64_t)1 << 39))
        return fail(ctx, "%s: too many sites x storm chunks for one launch; split the sites", who);
    const size_t n_tab = tab.size() + gch.size();

    if (w.d[0].grow(ctx, sizeof(Rec) * (size_t)std::max<int64_t>(1, n_trk * n_seg_max * kHzSeg)) < 0 ||
        w.d[1].grow(ctx, sizeof(HzCap) * (size_t)std::max<int64_t>(1, n_trk * (n_seg_max + 1))) < 0 ||
        w.d[2].grow(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(1, n_trk)) < 0 ||
        w.d[3].grow(ctx, sizeof(int32_t) * (size_t)std::max<int64_t>(1, n_chunk * n_site * n_bin)) < 0 ||
        w.d[4].grow(ctx, sizeof(int64_t) * (n_tab + 1)) < 0 ||
        (extra_bytes && w.d[5].grow(ctx, extra_bytes) < 0))
        return -1;
    // the chunk table goes up through a pinned buffer of the workspace; the previous call's upload must be done with it
    if (w.ev) HIPCHK(ctx, hipEventSynchronize(w.ev));
    else {
        HIPCHK(ctx, hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    }
    if (w.h.cap < n_tab) HIPCHK(ctx, w.h.alloc(n_tab));
    memcpy(w.h.p, tab.data(), tab.size() * sizeof(int64_t));
    memcpy(w.h.p + tab.size(), gch.data(), gch.size() * sizeof(int64_t));
    int64_t *d_tab = reinterpret_cast<int64_t *>(w.d[4].p);
    unsigned long long *d_pairs = reinterpret_cast<unsigned long long *>(d_tab + n_tab);
    HIPCHK(ctx, hipMemcpyAsync(d_tab, w.h.p, n_tab * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(w.ev, st));
    HIPCHK(ctx, hipMemsetAsync(d_pairs, 0, sizeof(unsigned long long), st));
    w.pairs = d_pairs;

    HzCap *caps = reinterpret_cast<HzCap *>(w.d[1].p);
    int32_t *part = reinterpret_cast<int32_t *>(w.d[3].p);
    if (n_trk > 0) {                                    // (then every storm is in a chunk: n_chunk > 0)
        ScanArgs<Rec> m{};
        m.rows = ScanRows<Rec>{reinterpret_cast<Rec *>(w.d[0].p), caps + n_trk, caps, reinterpret_cast<int32_t *>(w.d[2].p), n_seg_max};
        m.chunks = d_tab;
        m.site_lon = site_lon; m.site_lat = site_lat;
        m.n_site = n_site; m.n_tile = n_tile; m.n_trk = n_trk;
        m.a_R = scan_a_of(radius_km, re_km); m.r_ang = radius_km / re_km;
        m.n_bin = n_bin;
        for (int b = 0; b < n_bin; ++b) m.thr[b] = thresholds[b];
        m.part = part; m.site_max = site_max; m.pairs = d_pairs;
        HIPCHK(ctx, launch(m, w.d[5].p, dim3((unsigned)(n_tile * n_chunk)), sizeof(int32_t) * 64 * (n_bin + 1)));
    }
    const int64_t n_out = n_site * n_group * n_bin;
    hipLaunchKernelGGL(k_hazard_reduce, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, part, d_tab + tab.size(), n_site,
                       (int32_t)n_group, n_bin, counts);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(w.done, st));
    return 0;
}

// What a launch step enqueues: the analysis's prep kernel (one block of 64 lanes per storm) on p, then Policy's scan.
template <class Policy, class PrepArgs>
hipError_t scan_launch(void (*prep)(PrepArgs), const PrepArgs &p, int64_t n_trk, const ScanArgs<typename Policy::Rec> &m, dim3 grid,
                       size_t lds, hipStream_t st, const Policy &pol)
{
    hipLaunchKernelGGL(prep, dim3((unsigned)n_trk), dim3(64), 0, st, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_site_scan<Policy>, grid, dim3(64), lds, st, m, pol);
    return hipGetLastError();
}

// the sites and outputs of a _host entry point on the device (buffers of B), and the way back
struct ScanHostIO {
    const double *site_lon, *site_lat;
    int32_t *counts;
    double *site_max;
    size_t n_out, n_max;
    bool ok;
};

template <class Tracks>
ScanHostIO scan_host_io(DevBuf &B, const Tracks *t, int64_t n_site, const double *site_lon, const double *site_lat, int32_t n_bin,
                        bool want_max)
{
    ScanHostIO d{};
    d.site_lon = B.put(site_lon, (size_t)n_site); d.site_lat = B.put(site_lat, (size_t)n_site);
    d.n_out = (size_t)n_site * t->n_group * n_bin; d.n_max = (size_t)n_site * t->n_trk;
    d.counts = B.get<int32_t>(d.n_out);
    d.site_max = want_max ? B.get<double>((size_t)n_site * std::max<int64_t>(1, t->n_trk)) : nullptr;
    d.ok = d.site_lon && d.site_lat && d.counts && (!want_max || d.site_max);
    return d;
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
