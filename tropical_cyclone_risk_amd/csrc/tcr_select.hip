// Row selection behind the C ABI (include/tcrisk_hip.h, "row selection (return levels)" section): the ranks[j]-th largest value of
// every row of a [n_row][n_col] plane that is not NaN.  With return_period = total_years / count(peak >= v), the level of period T
// at a site is the k-th largest storm peak there, k the smallest integer with k T >= total_years: an order statistic of the
// site's row of a footprint's site_max / site_value plane, taken while the plane is still on the device.
//
//   k_row_select    one 256-thread workgroup per row.  One streaming pass maps the non-NaN values to order-preserving keys and
//                   compacts them into LDS (ballot + popcount, one LDS counter update per wave; the order inside LDS is
//                   irrelevant), counting them as it goes.  A row of at most TCR_SELECT_LDS_KEYS such values is then selected
//                   from LDS, a longer one from the row itself (360 KB for 45 000 storms, read once per pass: the rows in flight
//                   are more than L2 holds, which is what the global path costs);
//   sel_radix<Src>  the one selection routine of both: most-significant-digit radix select with 8-bit digits.  All ranks go
//                   through the eight passes together; ranks that still share a prefix share a histogram, and a pass sweeps the
//                   keys once per kSelBatch distinct prefixes.  Src is where key i comes from, and nothing else differs.
//
// The key of a double: its bits with every bit flipped when negative, the sign bit flipped otherwise, so that unsigned order is
// -inf < negatives < -0.0 < +0.0 < positives < +inf.  The result is the key mapped back: one of the row's own values, bit for
// bit; no arithmetic touches a value.

namespace {

constexpr int kSelThreads = 256;
constexpr int kSelUnroll = 8;                       // loads a lane has in flight, in the streaming pass and in a sweep over the keys
constexpr int kSelBatch = 8;                        // histograms (distinct prefixes) per sweep over the keys: 8 KB of LDS
constexpr int64_t kSelBlocksMax = 1 << 16;          // more rows than this: a workgroup takes several, one after the other
constexpr uint64_t kSelSign = 1ull << 63;
constexpr uint64_t kSelNaN = 0x7ff8000000000000ull;

__device__ __forceinline__ bool sel_is_nan(uint64_t bits) { return (bits & ~kSelSign) > 0x7ff0000000000000ull; }
__device__ __forceinline__ uint64_t sel_key(uint64_t bits) { return bits ^ ((bits & kSelSign) ? ~0ull : kSelSign); }
__device__ __forceinline__ uint64_t sel_bits(uint64_t key) { return key ^ ((key & kSelSign) ? kSelSign : ~0ull); }

// where key i of n comes from: the compacted keys in LDS (all present), or the row in global memory (a NaN is absent)
struct SelLdsKeys {
    const uint64_t *keys;
    __device__ __forceinline__ bool get(int64_t i, uint64_t *key) const { *key = keys[i]; return true; }
};
struct SelRowKeys {
    const uint64_t *row;
    __device__ __forceinline__ bool get(int64_t i, uint64_t *key) const
    {
        const uint64_t bits = row[i];
        *key = sel_key(bits);
        return !sel_is_nan(bits);
    }
};

struct SelArgs {
    const double *plane;
    int64_t n_row, n_col, stride;
    double *level;
    int32_t *n_valid;
    int32_t n_rank;
    int64_t ranks[TCR_SELECT_MAX_RANKS];
};

// the selection's state of one row, in LDS
struct SelState {
    uint64_t pre[TCR_SELECT_MAX_RANKS];             // the digits of rank j's key found so far (the key itself after pass 7)
    uint64_t lead[TCR_SELECT_MAX_RANKS];            // the distinct prefixes of the live ranks in this pass
    uint32_t rem[TCR_SELECT_MAX_RANKS];             // rank j is the rem-th largest of the keys that begin with pre; 0: no such value
    int32_t grp[TCR_SELECT_MAX_RANKS];              // the index in lead[] of rank j's prefix
    uint32_t hist[kSelBatch][256];
    int32_t n_lead;
    uint32_t count;
};

// Ranks st.rem[j] (1-based, descending; 0: absent) of the n keys of src -> st.pre[j].  Every thread of the workgroup calls it.
// Invariant of a live rank j before pass d: the keys whose top 8 d bits are pre[j] number at least rem[j], and the wanted key is
// the rem[j]-th largest of them.
template <typename Src>
__device__ void sel_radix(const Src &src, int64_t n, int n_rank, SelState &st)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int d = 0; d < 8; ++d) {
        const int shift = 56 - 8 * d;
        // the distinct prefixes (wave 0: rank j on lane j)
        if (wave == 0) {
            const bool live = lane < n_rank && st.rem[lane] > 0;
            const uint64_t pre = lane < n_rank ? st.pre[lane] : 0;
            bool first = live;
            for (int j = 0; j < lane && j < n_rank; ++j) first = first && !(st.rem[j] > 0 && st.pre[j] == pre);
            const unsigned long long m = __ballot(first);
            if (first) st.lead[__popcll(m & ((1ull << lane) - 1ull))] = pre;
            if (lane == 0) st.n_lead = __popcll(m);
        }
        __syncthreads();
        const int n_lead = st.n_lead;
        if (n_lead == 0) break;                             // every rank is past the row's count
        if (tid < n_rank && st.rem[tid] > 0) {
            int g = 0;
            while (g < n_lead - 1 && st.lead[g] != st.pre[tid]) ++g;        // (it is there: a live rank's prefix is a leader's)
            st.grp[tid] = g;
        }
        for (int g0 = 0; g0 < n_lead; g0 += kSelBatch) {
            const int nb = min(kSelBatch, n_lead - g0);
            for (int i = tid; i < nb * 256; i += kSelThreads) (&st.hist[0][0])[i] = 0;
            uint64_t lp[kSelBatch];
#pragma unroll
            for (int g = 0; g < kSelBatch; ++g) lp[g] = st.lead[g0 + min(g, nb - 1)];
            __syncthreads();
            // histogram of this digit under each prefix of the batch.  A wave makes the same number of turns on every lane (the
            // ballots below need every lane), and a lane has kSelUnroll keys in flight
            for (int64_t base = (int64_t)wave * 64; base < n; base += kSelUnroll * kSelThreads) {
                uint64_t key[kSelUnroll];
                bool ok[kSelUnroll];
#pragma unroll
                for (int u = 0; u < kSelUnroll; ++u) {
                    const int64_t i = base + u * kSelThreads + lane;
                    key[u] = 0;
                    ok[u] = i < n && src.get(i, &key[u]);
                }
#pragma unroll
                for (int u = 0; u < kSelUnroll; ++u) {
                    const uint64_t hi = d ? key[u] >> (shift + 8) : 0;
                    int bin = -1;
#pragma unroll
                    for (int g = 0; g < kSelBatch; ++g)
                        if (g < nb && hi == lp[g]) bin = g * 256 + (int)((key[u] >> shift) & 255);
                    if (!ok[u]) bin = -1;
                    // values of one magnitude share their leading digits: one update for the wave when every lane has the same bin
                    const int bin0 = __builtin_amdgcn_readfirstlane(bin);
                    if (__all(bin == bin0)) {
                        if (bin0 >= 0 && lane == 0) atomicAdd(&st.hist[0][0] + bin0, 64u);
                    } else if (bin >= 0) {
                        atomicAdd(&st.hist[0][0] + bin, 1u);
                    }
                }
            }
            __syncthreads();
            // hist[g][t] <- the number of keys under prefix g with digit >= t (wave w: histograms w, w + 4; lane l: bins 4 l .. 4 l + 3)
            for (int g = wave; g < nb; g += kSelThreads / 64) {
                uint32_t *h = st.hist[g] + 4 * lane;
                const uint32_t s3 = h[3], s2 = s3 + h[2], s1 = s2 + h[1], s0 = s1 + h[0];
                uint32_t above = s0;                        // inclusive suffix sum over the lanes, then minus the lane's own
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t v = __shfl_down(above, o, 64);
                    if (lane + o < 64) above += v;
                }
                above -= s0;
                h[0] = s0 + above; h[1] = s1 + above; h[2] = s2 + above; h[3] = s3 + above;
            }
            __syncthreads();
            // rank j's digit: the largest t with hist[t] >= rem (hist[0] >= rem by the invariant)
            if (tid < n_rank && st.rem[tid] > 0 && st.grp[tid] >= g0 && st.grp[tid] < g0 + nb) {
                const uint32_t *h = st.hist[st.grp[tid] - g0];
                const uint32_t rem = st.rem[tid];
                int lo = 0, top = 255;
                while (lo < top) {
                    const int mid = (lo + top + 1) >> 1;
                    if (h[mid] >= rem) lo = mid; else top = mid - 1;
                }
                st.pre[tid] = (st.pre[tid] << 8) | (uint64_t)lo;
                st.rem[tid] = rem - (lo < 255 ? h[lo + 1] : 0u);
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kSelThreads) void k_row_select(SelArgs a)
{
    __shared__ uint64_t keys[TCR_SELECT_LDS_KEYS];
    __shared__ SelState st;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t r = blockIdx.x; r < a.n_row; r += gridDim.x) {
        const uint64_t *row = reinterpret_cast<const uint64_t *>(a.plane) + r * a.stride;
        if (tid == 0) st.count = 0;
        __syncthreads();
        // one pass over the row: the keys of the values that are not NaN go to LDS while there is room, and are counted
        for (int64_t base = (int64_t)(tid - lane); base < a.n_col; base += kSelUnroll * kSelThreads) {
            uint64_t bits[kSelUnroll];
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u) {
                const int64_t i = base + u * kSelThreads + lane;
                bits[u] = i < a.n_col ? row[i] : kSelNaN;
            }
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u) {
                const bool live = !sel_is_nan(bits[u]);
                const unsigned long long m = __ballot(live);
                if (m) {
                    uint32_t at = 0;
                    if (lane == 0) at = atomicAdd(&st.count, (uint32_t)__popcll(m));
                    at = __shfl(at, 0, 64) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    if (live && at < (uint32_t)TCR_SELECT_LDS_KEYS) keys[at] = sel_key(bits[u]);
                }
            }
        }
        __syncthreads();
        const uint32_t count = st.count;
        if (tid < a.n_rank) {
            st.pre[tid] = 0;
            st.rem[tid] = a.ranks[tid] <= (int64_t)count ? (uint32_t)a.ranks[tid] : 0u;
        }
        __syncthreads();
        if (count <= (uint32_t)TCR_SELECT_LDS_KEYS) sel_radix(SelLdsKeys{keys}, (int64_t)count, a.n_rank, st);
        else sel_radix(SelRowKeys{row}, a.n_col, a.n_rank, st);
        if (tid < a.n_rank) {
            const uint64_t out = st.rem[tid] > 0 ? sel_bits(st.pre[tid]) : kSelNaN;
            reinterpret_cast<uint64_t *>(a.level)[r * a.n_rank + tid] = out;
        }
        if (tid == 0 && a.n_valid) a.n_valid[r] = (int32_t)count;
        __syncthreads();
    }
}

int select_check(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, int32_t n_rank,
                 const int64_t *ranks, const double *level)
{
    if (!ranks || !level || (n_row > 0 && !plane)) return fail(ctx, "tcr_select: NULL argument");
    if (n_row < 0) return fail(ctx, "tcr_select: n_row must be >= 0");
    if (n_col < 1 || n_col > INT32_MAX) return fail(ctx, "tcr_select: n_col must be in [1, 2^31 - 1]");
    if (row_stride < n_col) return fail(ctx, "tcr_select: row_stride must be >= n_col");
    if (n_row > 1 && row_stride > INT64_MAX / (8 * n_row)) return fail(ctx, "tcr_select: the plane is too large");
    if (n_rank < 1 || n_rank > TCR_SELECT_MAX_RANKS) return fail(ctx, "tcr_select: n_rank must be in [1, 64]");
    for (int j = 0; j < n_rank; ++j)
        if (ranks[j] < 1) return fail(ctx, "tcr_select: ranks must be >= 1");
    return 0;
}

}  // namespace

extern "C" {

int tcr_select_dev(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, int32_t n_rank,
                   const int64_t *ranks, double *level, int32_t *n_valid, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || select_check(ctx, plane, n_row, n_col, row_stride, n_rank, ranks, level)) return -1;
    if (n_row == 0) return 0;
    SelArgs a{};
    a.plane = plane; a.n_row = n_row; a.n_col = n_col; a.stride = row_stride; a.level = level; a.n_valid = n_valid; a.n_rank = n_rank;
    for (int j = 0; j < n_rank; ++j) a.ranks[j] = ranks[j];
    hipLaunchKernelGGL(k_row_select, dim3((unsigned)std::min(n_row, kSelBlocksMax)), dim3(kSelThreads), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int tcr_select_host(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, int32_t n_rank,
                    const int64_t *ranks, double *level, int32_t *n_valid)
{
    if (!enter(ctx) || select_check(ctx, plane, n_row, n_col, row_stride, n_rank, ranks, level)) return -1;
    if (n_row == 0) return 0;
    DevBuf B;
    const size_t n_in = (size_t)(n_row - 1) * (size_t)row_stride + (size_t)n_col, n_out = (size_t)n_row * (size_t)n_rank;
    const double *d_plane = B.put(plane, n_in);
    double *d_level = B.get<double>(n_out);
    int32_t *d_valid = B.get<int32_t>((size_t)n_row);
    if (!d_plane || !d_level || !d_valid) return fail(ctx, "tcr_select_host: device allocation / upload failed");
    if (tcr_select_dev(ctx, d_plane, n_row, n_col, row_stride, n_rank, ranks, d_level, d_valid, ctx->stream)) return -1;
    HIPCHK(ctx, hipMemcpyAsync(level, d_level, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
    if (n_valid) HIPCHK(ctx, hipMemcpyAsync(n_valid, d_valid, sizeof(int32_t) * (size_t)n_row, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
