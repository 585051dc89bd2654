// Joint hazard behind the C ABI (include/tcrisk_hip.h, "joint hazard (co-exceedance between sites)" section): one bit per (row,
// level, unit) says "this unit reached this level in this row", and the number of units that reached a level in two rows at once
// is the popcount of the AND of their bit rows.  It is what turns the per-storm plane of a site analysis (site_max, site_total,
// ...) into co-exceedance counts between sites, per storm or per year, while the plane of a block of sites is on the device.
//
//   k_joint_pack          identity units (unit = column).  The sweep of k_rowpack_count: one 256-thread workgroup per row (several
//                         rows in turn past kJointBlocksMax), wave w takes the kJointUnroll runs of 64 columns from w x 64 x
//                         kJointUnroll on.  A run of 64 columns is one output word, and the ballot of value >= level is that word:
//                         lane l keeps the word of level l, and one vector store of the lanes below n_level writes a run's words of
//                         every level.  All levels are compared on the one load of a value.  The popcounts of the words meet in
//                         LDS (integer sums) and lane l of the first wave writes n_set[l][r].
//   k_joint_pack_mapped   units through unit_of.  The same sweep; a hit is an LDS atomic OR into a zeroed image of the row,
//                         n_word words per level, for as many levels at a time as kJointImageWords holds (all of them, or a
//                         loop over groups of levels, each with a sweep of its own).  After a barrier the image is copied out
//                         and counted.  OR and integer sums do not depend on their order: the result is a function of the inputs.
//   k_joint_cross         one 256-thread workgroup per 64 x 64 tile of counts[l].  Both tiles of kJointKW words are staged into
//                         LDS word-major (tile[w][row], rows padded to kJointLd words so that the 16 words a quarter wave stores
//                         fall into different banks); thread (ty, tx) owns rows 4 ty .. 4 ty + 3 of a, read as two 16-byte reads of
//                         32 adjacent bytes (one address per quarter wave: a broadcast), and columns 2 tx, 2 tx + 1, 32 + 2 tx,
//                         33 + 2 tx of b, two 16-byte reads that are each 256 adjacent bytes over the 16 tx (four adjacent
//                         columns per thread would put tx and tx + 8 on the same banks).  Per word and cell: the AND and the
//                         popcount-accumulate of the two 32-bit halves.  Rows past n_a / n_b and words past n_word are zero in
//                         LDS; cells past the edge are not stored.
//
// No floating-point atomics, no global atomics, no workspace: calls on one context need no ordering.

namespace {

constexpr int kJointThreads = 256;
constexpr int kJointWaves = kJointThreads / 64;
constexpr int kJointUnroll = TCR_ROWPACK_UNROLL;          // loads a lane has in flight (k_rowpack_count's)
constexpr int kJointSpan = 64 * kJointUnroll;             // adjacent columns of one wave in a turn
constexpr int kJointTurn = kJointThreads * kJointUnroll;  // columns of one turn of the workgroup
constexpr int64_t kJointBlocksMax = 1 << 16;              // more rows than this: a workgroup takes several, one after the other
constexpr int kJointMaxLevels = TCR_JOINT_MAX_LEVELS;
constexpr int kJointImageWords = 4096;                    // the LDS image of k_joint_pack_mapped: 32 KB, one level of 2^18 units
constexpr int kJointKW = TCR_JOINT_KW;                    // words of a row k_joint_cross stages per chunk
constexpr int kJointTile = 64;                            // rows of a and of b per workgroup
constexpr int kJointLd = kJointTile + 2;                  // words from tile[w][0] to tile[w + 1][0] (even: 16-byte reads stay aligned)
constexpr uint64_t kJointNaN = 0x7ff8000000000000ull;
constexpr int64_t kJointHostMaxBytes = (int64_t)1 << 32;  // what tcr_joint_host puts on the device at most

static_assert(kJointMaxLevels <= 64, "a lane per level");
static_assert(TCR_JOINT_MAX_MAPPED_UNITS <= 64 * kJointImageWords, "one level of the largest mapped row fits the image");
static_assert(kJointLd % 2 == 0 && kJointTile == 64 && kJointThreads == 256, "k_joint_cross: 16 x 16 threads of 4 x 4 cells");
static_assert(kJointThreads % kJointKW == 0 && kJointTile % (kJointThreads / kJointKW) == 0, "k_joint_cross: whole staging passes");

__device__ __forceinline__ bool joint_reach(uint64_t bits, double level) { return __longlong_as_double((long long)bits) >= level; }

__global__ __launch_bounds__(kJointThreads) void k_joint_pack(const double *plane, int64_t n_row, int64_t n_col, int64_t stride,
                                                              const double *level, int n_level, uint64_t *bits, int64_t n_word,
                                                              int64_t level_stride, int32_t *n_set, int64_t n_set_stride)
{
    __shared__ double s_lev[kJointMaxLevels];
    __shared__ int32_t tot[kJointWaves][kJointMaxLevels];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t r = blockIdx.x; r < n_row; r += gridDim.x) {
        const uint64_t *row = reinterpret_cast<const uint64_t *>(plane) + r * stride;
        // (s_lev was last read before the second barrier of the row before, tot before this one)
        if (tid < n_level) s_lev[tid] = level[r * n_level + tid];
        __syncthreads();
        int32_t n = 0;                                      // lane l: units of level l this wave has seen
        for (int64_t base = (int64_t)wave * kJointSpan; base < n_col; base += kJointTurn) {
            uint64_t v[kJointUnroll];
            unsigned long long mine[kJointUnroll];
#pragma unroll
            for (int u = 0; u < kJointUnroll; ++u) {
                const int64_t i = base + u * 64 + lane;
                v[u] = i < n_col ? row[i] : kJointNaN;
                mine[u] = 0;
            }
            for (int l = 0; l < n_level; ++l) {
                const double lev = s_lev[l];
#pragma unroll
                for (int u = 0; u < kJointUnroll; ++u) {
                    const unsigned long long m = __ballot(joint_reach(v[u], lev));
                    mine[u] = lane == l ? m : mine[u];
                }
            }
            if (lane < n_level) {
                uint64_t *out = bits + (int64_t)lane * level_stride + r * n_word + (base >> 6);
#pragma unroll
                for (int u = 0; u < kJointUnroll; ++u)
                    if (base + u * 64 < n_col) {            // (a run that begins in the row is one of its n_word words)
                        out[u] = mine[u];
                        n += __popcll(mine[u]);
                    }
            }
        }
        if (lane < n_level) tot[wave][lane] = n;
        __syncthreads();
        if (n_set && tid < n_level) n_set[(int64_t)tid * n_set_stride + r] = tot[0][tid] + tot[1][tid] + tot[2][tid] + tot[3][tid];
    }
}

// LDS, all of it dynamic (16-byte aligned carve): s_lev [kJointMaxLevels] fp64, tot [kJointMaxLevels] int32, then the image
// [n_pass][n_word] uint64, n_pass the levels of one sweep.
__global__ __launch_bounds__(kJointThreads) void k_joint_pack_mapped(const double *plane, int64_t n_row, int64_t n_col, int64_t stride,
                                                                     const double *level, int n_level, const int32_t *unit_of,
                                                                     int64_t n_unit, uint64_t *bits, int n_word, int64_t level_stride,
                                                                     int32_t *n_set, int64_t n_set_stride, int n_pass)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char joint_lds[];
    double *s_lev = reinterpret_cast<double *>(joint_lds);
    int32_t *tot = reinterpret_cast<int32_t *>(joint_lds + sizeof(double) * kJointMaxLevels);
    unsigned long long *img = reinterpret_cast<unsigned long long *>(joint_lds + (sizeof(double) + sizeof(int32_t)) * kJointMaxLevels);
    const int tid = threadIdx.x;
    for (int64_t r = blockIdx.x; r < n_row; r += gridDim.x) {
        const uint64_t *row = reinterpret_cast<const uint64_t *>(plane) + r * stride;
        // (the last reads of s_lev and tot of the row before are behind its last barrier)
        if (tid < n_level) {
            s_lev[tid] = level[r * n_level + tid];
            tot[tid] = 0;
        }
        for (int l0 = 0; l0 < n_level; l0 += n_pass) {
            const int nl = min(n_pass, n_level - l0);
            for (int i = tid; i < nl * n_word; i += kJointThreads) img[i] = 0;
            __syncthreads();
            for (int64_t base = (int64_t)tid; base < n_col; base += kJointTurn) {
                uint64_t v[kJointUnroll];
                int32_t un[kJointUnroll];
#pragma unroll
                for (int u = 0; u < kJointUnroll; ++u) {
                    const int64_t i = base + (int64_t)u * kJointThreads;
                    v[u] = i < n_col ? row[i] : kJointNaN;
                    un[u] = i < n_col ? unit_of[i] : -1;
                }
#pragma unroll
                for (int u = 0; u < kJointUnroll; ++u) {
                    if ((uint64_t)(int64_t)un[u] >= (uint64_t)n_unit) continue;        // (a unit out of range sets no bit)
                    const unsigned long long bit = 1ull << (un[u] & 63);
                    for (int l = 0; l < nl; ++l)
                        if (joint_reach(v[u], s_lev[l0 + l])) atomicOr(&img[l * n_word + (un[u] >> 6)], bit);
                }
            }
            __syncthreads();
            for (int l = 0; l < nl; ++l) {
                uint64_t *out = bits + (int64_t)(l0 + l) * level_stride + r * n_word;
                int32_t n = 0;
                for (int i = tid; i < n_word; i += kJointThreads) {
                    const unsigned long long w = img[l * n_word + i];
                    out[i] = w;
                    n += __popcll(w);
                }
                if (n) atomicAdd(&tot[l0 + l], n);
            }
            __syncthreads();                                // (the image is zeroed again, or tot read, behind this)
        }
        if (n_set && tid < n_level) n_set[(int64_t)tid * n_set_stride + r] = tot[tid];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kJointThreads) void k_joint_cross(const uint64_t *a, int64_t n_a, int64_t a_level_stride, const uint64_t *b,
                                                               int64_t n_b, int64_t b_level_stride, int64_t n_word, int32_t *counts)
{
    __shared__ __attribute__((aligned(16))) uint64_t sa[kJointKW * kJointLd];
    __shared__ __attribute__((aligned(16))) uint64_t sb[kJointKW * kJointLd];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t j0 = (int64_t)blockIdx.x * kJointTile, i0 = (int64_t)blockIdx.y * kJointTile, l = blockIdx.z;
    const uint64_t *al = a + l * a_level_stride, *bl = b + l * b_level_stride;
    // staging: thread t takes word t % kJointKW of the rows t / kJointKW + k x (256 / kJointKW): a wave reads whole runs of a row
    const int sw = tid % kJointKW, sr = tid / kJointKW;
    constexpr int kRowsPerPass = kJointThreads / kJointKW, kPasses = kJointTile / kRowsPerPass;
    int32_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0;
    for (int64_t w0 = 0; w0 < n_word; w0 += kJointKW) {
        uint64_t ga[kPasses], gb[kPasses];
        const bool in_w = w0 + sw < n_word;
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            const int64_t ra = i0 + sr + k * kRowsPerPass, rb = j0 + sr + k * kRowsPerPass;
            ga[k] = in_w && ra < n_a ? al[ra * n_word + w0 + sw] : 0;
            gb[k] = in_w && rb < n_b ? bl[rb * n_word + w0 + sw] : 0;
        }
        __syncthreads();                                    // (the chunk before has been read)
#pragma unroll
        for (int k = 0; k < kPasses; ++k) {
            sa[sw * kJointLd + sr + k * kRowsPerPass] = ga[k];
            sb[sw * kJointLd + sr + k * kRowsPerPass] = gb[k];
        }
        __syncthreads();
#pragma unroll 4
        for (int w = 0; w < kJointKW; ++w) {
            const ulonglong2 a01 = *reinterpret_cast<const ulonglong2 *>(&sa[w * kJointLd + 4 * ty]);
            const ulonglong2 a23 = *reinterpret_cast<const ulonglong2 *>(&sa[w * kJointLd + 4 * ty + 2]);
            const ulonglong2 b01 = *reinterpret_cast<const ulonglong2 *>(&sb[w * kJointLd + 2 * tx]);
            const ulonglong2 b23 = *reinterpret_cast<const ulonglong2 *>(&sb[w * kJointLd + 32 + 2 * tx]);
            const uint64_t av[4] = {a01.x, a01.y, a23.x, a23.y}, bv[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint64_t x = av[i] & bv[j];
                    acc[i][j] += __popc((uint32_t)x) + __popc((uint32_t)(x >> 32));
                }
        }
    }
    int32_t *cl = counts + l * n_a * n_b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t ri = i0 + 4 * ty + i;
        if (ri >= n_a) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t cj = j0 + (j < 2 ? 2 * tx + j : 32 + 2 * tx + (j - 2));
            if (cj < n_b) cl[ri * n_b + cj] = acc[i][j];
        }
    }
}

int64_t joint_words(int64_t n_unit) { return (n_unit + 63) / 64; }

// The checks of a pack.  host: level and unit_of are host memory, and their entries are checked too.
int joint_pack_check(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, const double *level,
                     int32_t n_level, const int32_t *unit_of, int64_t n_unit, int64_t level_stride, int64_t n_set_stride, bool have_n_set,
                     bool host)
{
    if (n_row > 0 && (!plane || !level)) return fail(ctx, "tcr_joint: NULL argument");
    if (n_row < 0) return fail(ctx, "tcr_joint: n_row must be >= 0");
    if (n_col < 1 || n_col > INT32_MAX) return fail(ctx, "tcr_joint: n_col must be in [1, 2^31 - 1]");
    if (row_stride < n_col) return fail(ctx, "tcr_joint: row_stride must be >= n_col");
    if (n_row > 1 && row_stride > INT64_MAX / (8 * n_row)) return fail(ctx, "tcr_joint: the plane is too large");
    if (n_level < 1 || n_level > kJointMaxLevels) return fail(ctx, "tcr_joint: n_level must be in [1, 16]");
    if (unit_of) {
        if (n_unit < 1 || n_unit > TCR_JOINT_MAX_MAPPED_UNITS) return fail(ctx, "tcr_joint: with unit_of, n_unit must be in [1, 2^18]");
    } else if (n_unit != n_col) return fail(ctx, "tcr_joint: without unit_of, n_unit must be n_col");
    const int64_t n_word = joint_words(n_unit);
    if (n_row > 0 && n_word > INT64_MAX / (8 * (int64_t)kJointMaxLevels) / n_row) return fail(ctx, "tcr_joint: the bit table is too large");
    if (level_stride < n_row * n_word) return fail(ctx, "tcr_joint: level_stride must be >= n_row x n_word");
    if (level_stride > INT64_MAX / (8 * (int64_t)kJointMaxLevels)) return fail(ctx, "tcr_joint: the bit table is too large");
    if (have_n_set && (n_set_stride < n_row || n_set_stride > INT64_MAX / (4 * (int64_t)kJointMaxLevels)))
        return fail(ctx, "tcr_joint: n_set_stride must be >= n_row");
    if (host)
        for (int64_t i = 0; i < n_row * n_level; ++i)
            if (level[i] != level[i]) return fail(ctx, "tcr_joint: a level is NaN");
    if (host && unit_of)
        for (int64_t c = 0; c < n_col; ++c)
            if (unit_of[c] < 0 || unit_of[c] >= n_unit) return fail(ctx, "tcr_joint: an entry of unit_of is not in [0, n_unit)");
    return 0;
}

}  // namespace

extern "C" {

int tcr_joint_pack_dev(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, const double *level,
                       int32_t n_level, const int32_t *unit_of, int64_t n_unit, uint64_t *bits, int64_t level_stride, int32_t *n_set,
                       int64_t n_set_stride, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || joint_pack_check(ctx, plane, n_row, n_col, row_stride, level, n_level, unit_of, n_unit, level_stride, n_set_stride,
                                n_set != nullptr, false))
        return -1;
    if (n_row == 0) return 0;
    if (!bits) return fail(ctx, "tcr_joint: NULL argument");
    const int64_t n_word = joint_words(n_unit);
    const dim3 grid((unsigned)std::min(n_row, kJointBlocksMax));
    if (!unit_of) {
        hipLaunchKernelGGL(k_joint_pack, grid, dim3(kJointThreads), 0, st, plane, n_row, n_col, row_stride, level, (int)n_level, bits,
                           n_word, level_stride, n_set, n_set_stride);
    } else {
        const int n_pass = (int)std::min<int64_t>(n_level, kJointImageWords / n_word);
        const size_t lds = (sizeof(double) + sizeof(int32_t)) * kJointMaxLevels + sizeof(uint64_t) * (size_t)n_pass * (size_t)n_word;
        hipLaunchKernelGGL(k_joint_pack_mapped, grid, dim3(kJointThreads), lds, st, plane, n_row, n_col, row_stride, level, (int)n_level,
                           unit_of, n_unit, bits, (int)n_word, level_stride, n_set, n_set_stride, n_pass);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int tcr_joint_cross_dev(tcr_ctx *ctx, const uint64_t *a_bits, int64_t n_a, int64_t a_level_stride, const uint64_t *b_bits, int64_t n_b,
                        int64_t b_level_stride, int64_t n_word, int32_t n_level, int32_t *counts, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    if (n_a < 0 || n_b < 0) return fail(ctx, "tcr_joint: n_a and n_b must be >= 0");
    if (n_level < 1 || n_level > kJointMaxLevels) return fail(ctx, "tcr_joint: n_level must be in [1, 16]");
    if (n_word < 0 || n_word > (int64_t)INT32_MAX / 64 + 1) return fail(ctx, "tcr_joint: n_word must be in [0, 2^25]");
    if (n_a == 0 || n_b == 0) return 0;
    if (!counts || (n_word > 0 && (!a_bits || !b_bits))) return fail(ctx, "tcr_joint: NULL argument");
    const int64_t tiles_a = (n_a + kJointTile - 1) / kJointTile, tiles_b = (n_b + kJointTile - 1) / kJointTile;
    if (tiles_a > 65535) return fail(ctx, "tcr_joint: n_a must be <= 65535 x 64 (cross the rows of a in parts)");
    if (tiles_b >= (int64_t)1 << 24) return fail(ctx, "tcr_joint: n_b must be < 2^30");
    if (n_a > INT64_MAX / (4 * (int64_t)kJointMaxLevels) / n_b) return fail(ctx, "tcr_joint: the counts are too large");
    const int64_t lim = INT64_MAX / (8 * (int64_t)kJointMaxLevels);
    if (a_level_stride < n_a * n_word || b_level_stride < n_b * n_word || a_level_stride > lim || b_level_stride > lim)
        return fail(ctx, "tcr_joint: a level stride must be >= the rows of its table x n_word");
    hipLaunchKernelGGL(k_joint_cross, dim3((unsigned)tiles_b, (unsigned)tiles_a, (unsigned)n_level), dim3(kJointThreads), 0, st, a_bits, n_a,
                       a_level_stride, b_bits, n_b, b_level_stride, n_word, counts);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int tcr_joint_host(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, const double *level,
                   int32_t n_level, const int32_t *unit_of, int64_t n_unit, int32_t *counts, int32_t *n_set)
{
    if (!enter(ctx)) return -1;
    if (!counts && n_row > 0) return fail(ctx, "tcr_joint: NULL argument");
    const int64_t n_word = n_unit > 0 ? joint_words(n_unit) : 0;
    // (the table is packed at its own size: level_stride = n_row x n_word.  A product that overflows fails the check's own test.)
    const int64_t level_stride = n_row > 0 && n_word <= INT64_MAX / (8 * (int64_t)kJointMaxLevels) / n_row ? n_row * n_word : -1;
    if (joint_pack_check(ctx, plane, n_row, n_col, row_stride, level, n_level, unit_of, n_unit, n_row > 0 ? level_stride : 0, n_row,
                         n_set != nullptr, true))
        return -1;
    if (n_row == 0) return 0;
    // the size of everything the call puts on the device, in fp64 first: no product below can overflow once it has passed
    const double need = 8.0 * (double)n_row * (double)row_stride + 8.0 * (double)n_level * (double)n_row * (double)n_word +
                        4.0 * (double)n_level * (double)n_row * (double)n_row;
    if (need > (double)kJointHostMaxBytes)
        return fail(ctx, "tcr_joint: plane, bit table and counts are more than 2^32 bytes: too large for tcr_joint_host (pack and cross blocks with the _dev entry points)");
    DevBuf B;
    const size_t n_in = (size_t)(n_row - 1) * (size_t)row_stride + (size_t)n_col;
    const double *d_plane = B.put(plane, n_in);
    const double *d_level = B.put(level, (size_t)n_row * (size_t)n_level);
    const int32_t *d_unit = unit_of ? B.put(unit_of, (size_t)n_col) : nullptr;
    uint64_t *d_bits = B.get<uint64_t>((size_t)n_level * (size_t)level_stride);
    int32_t *d_counts = B.get<int32_t>((size_t)n_level * (size_t)n_row * (size_t)n_row);
    int32_t *d_set = B.get<int32_t>((size_t)n_level * (size_t)n_row);
    if (!d_plane || !d_level || (unit_of && !d_unit) || !d_bits || !d_counts || !d_set)
        return fail(ctx, "tcr_joint: device allocation / upload failed");
    if (tcr_joint_pack_dev(ctx, d_plane, n_row, n_col, row_stride, d_level, n_level, d_unit, n_unit, d_bits, level_stride, d_set, n_row,
                           ctx->stream))
        return -1;
    if (tcr_joint_cross_dev(ctx, d_bits, n_row, level_stride, d_bits, n_row, level_stride, n_word, n_level, d_counts, ctx->stream)) return -1;
    HIPCHK(ctx, hipMemcpyAsync(counts, d_counts, sizeof(int32_t) * (size_t)n_level * (size_t)n_row * (size_t)n_row, hipMemcpyDeviceToHost,
                               ctx->stream));
    if (n_set)
        HIPCHK(ctx, hipMemcpyAsync(n_set, d_set, sizeof(int32_t) * (size_t)n_level * (size_t)n_row, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
