// Row tail fit behind the C ABI (include/tcrisk_hip.h, "row tail fit (return levels past the record)" section): per row of a
// [n_row][n_col] plane, a generalized Pareto distribution fitted to the excesses of the k largest values over the (k+1)-th, and
// the levels of any return periods read off the fit.  Included after tcr_select.hip: the keys, the streaming compaction and
// sel_radix are that file's.
//
//   k_row_tail      one 256-thread workgroup per row.  The same streaming compaction into LDS and the same count as
//                   k_row_select; sel_radix with the single rank k + 1, from LDS or from the row exactly as k_row_select chooses:
//                   the threshold u.  The keys strictly above u's (at most k of them) are gathered into the front of the key buffer
//                   (ballot + popcount), the rest of the k entries filled with u's key, the buffer padded to a power of two with
//                   the all-ones key (no value's) and sorted ascending by a bitonic network.  Keys back to values, excesses, the
//                   two sums with the header's fixed pairing, the probability-weighted-moment estimators, and lanes 0 .. n_T - 1
//                   evaluate the levels.
//
// LDS: the key buffer and the selection state of k_row_select and 80 bytes more, so two workgroups share a CU as there.  The sort
// buffer is the key buffer itself: once u is known the compacted keys are needed only once more, for the gather.  On the LDS path
// the first TCR_TAIL_MAX_K keys are taken into registers (8 per thread) before anything is written, and every write of the gather
// lands below TCR_TAIL_MAX_K, where nothing is read any more; on the global path the buffer holds nothing that is still needed.
//
// The sums: element j of the padded array belongs to thread j / 8.  A thread adds its eight as ((0+1)+(2+3))+((4+5)+(6+7)), the
// lanes of a wave combine by xor-butterfly (lane l with l ^ 1, l ^ 2, ...: IEEE addition commutes, so both lanes of a pair hold
// the pair's sum), the four waves as (0+1)+(2+3): the tree s[i] = s[2i] + s[2i+1] over 2048 entries.  The entries past the
// header's P are +0.0 and no partial sum is -0.0 (an excess is x - u with x >= u), so this is the tree over P entries, bit for bit.

namespace {

static_assert(kSelUnroll * kSelThreads >= TCR_TAIL_MAX_K, "the gather's register stage must cover the sort buffer");
static_assert(TCR_TAIL_MAX_K == 8 * kSelThreads, "the sums give eight entries to a thread");
static_assert(TCR_TAIL_MAX_K <= TCR_SELECT_LDS_KEYS, "the sort buffer is the front of the key buffer");

constexpr uint64_t kTailPad = ~0ull;                // sorts after every value's key (the key of a NaN with all bits set)

// The key sources of k_row_select under names of this kernel's own: sel_radix<Src> is then instantiated once per kernel and each
// instance has one caller, so the compiler goes on inlining k_row_select's into it (a routine with two callers becomes a called
// function with a stack frame, in both kernels).
struct TailLdsKeys : SelLdsKeys {};
struct TailRowKeys : SelRowKeys {};

struct TailArgs {
    const double *plane;
    int64_t n_row, n_col, stride;
    double *param, *level;
    int32_t *n_valid;
    int32_t k, n_period;
    double L[TCR_SELECT_MAX_RANKS];                 // log((k / total_years) T_j), from the host
};

// one wave-instruction of the gather: the lanes whose key is above the threshold append it to buf (any order)
__device__ __forceinline__ void tail_push(bool above, uint64_t key, uint64_t *buf, uint32_t *counter, int lane)
{
    const unsigned long long m = __ballot(above);
    if (m) {
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(counter, (uint32_t)__popcll(m));
        at = __shfl(at, 0, 64) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (above && at < (uint32_t)TCR_TAIL_MAX_K) buf[at] = key;
    }
}

__global__ __launch_bounds__(kSelThreads) void k_row_tail(TailArgs a)
{
    __shared__ uint64_t keys[TCR_SELECT_LDS_KEYS];
    __shared__ SelState st;
    __shared__ double part[2][kSelThreads / 64];
    __shared__ uint32_t n_above;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k;
    int P = 2;
    while (P < k) P <<= 1;
    for (int64_t r = blockIdx.x; r < a.n_row; r += gridDim.x) {
        const uint64_t *row = reinterpret_cast<const uint64_t *>(a.plane) + r * a.stride;
        uint64_t *param = reinterpret_cast<uint64_t *>(a.param) + 3 * r;
        uint64_t *level = reinterpret_cast<uint64_t *>(a.level) + r * a.n_period;
        if (tid == 0) { st.count = 0; n_above = 0; }
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
        const bool in_lds = count <= (uint32_t)TCR_SELECT_LDS_KEYS;
        if (tid == 0) {
            st.pre[0] = 0;
            st.rem[0] = (uint32_t)k + 1u <= count ? (uint32_t)k + 1u : 0u;
            if (a.n_valid) a.n_valid[r] = (int32_t)count;
        }
        __syncthreads();
        // the threshold: the (k+1)-th largest
        if (in_lds) sel_radix(TailLdsKeys{{keys}}, (int64_t)count, 1, st);
        else sel_radix(TailRowKeys{{row}}, a.n_col, 1, st);
        const bool have = st.rem[0] > 0;                        // (the same on every thread)
        const uint64_t ukey = st.pre[0];
        if (!have) {
            if (tid < 3) param[tid] = kSelNaN;
            if (tid < a.n_period) level[tid] = kSelNaN;
            __syncthreads();
            continue;
        }
        // the keys above the threshold's -> keys[0 .. n_above), n_above <= k
        if (in_lds) {
            uint64_t head[kSelUnroll];
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u) {
                const uint32_t i = (uint32_t)(u * kSelThreads + tid);
                head[u] = i < count ? keys[i] : 0ull;           // (key 0 is no value's, and above no threshold)
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u) tail_push(head[u] > ukey, head[u], keys, &n_above, lane);
            for (uint32_t base = (uint32_t)(kSelUnroll * kSelThreads + wave * 64); base < count; base += kSelUnroll * kSelThreads) {
                uint64_t key[kSelUnroll];
#pragma unroll
                for (int u = 0; u < kSelUnroll; ++u) {
                    const uint32_t i = base + (uint32_t)(u * kSelThreads + lane);
                    key[u] = i < count ? keys[i] : 0ull;
                }
#pragma unroll
                for (int u = 0; u < kSelUnroll; ++u) tail_push(key[u] > ukey, key[u], keys, &n_above, lane);
            }
        } else {
            for (int64_t base = (int64_t)(tid - lane); base < a.n_col; base += kSelUnroll * kSelThreads) {
                uint64_t bits[kSelUnroll];
#pragma unroll
                for (int u = 0; u < kSelUnroll; ++u) {
                    const int64_t i = base + u * kSelThreads + lane;
                    bits[u] = i < a.n_col ? row[i] : kSelNaN;
                }
#pragma unroll
                for (int u = 0; u < kSelUnroll; ++u) {
                    const uint64_t key = sel_key(bits[u]);
                    tail_push(!sel_is_nan(bits[u]) && key > ukey, key, keys, &n_above, lane);
                }
            }
        }
        __syncthreads();
        // ties at the threshold until there are k, then the padding of the sort
        for (int i = (int)min(n_above, (uint32_t)k) + tid; i < P; i += kSelThreads) keys[i] = i < k ? ukey : kTailPad;
        __syncthreads();
        // bitonic sort of keys[0 .. P), ascending
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < P / 2; t += kSelThreads) {
                    const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                    const uint64_t lo = keys[i], hi = keys[j];
                    if ((lo > hi) == ((i & size) == 0)) { keys[i] = hi; keys[j] = lo; }
                }
                __syncthreads();
            }
        }
        // excesses y_1 <= ... <= y_k and the two sums
        const double uval = __longlong_as_double((long long)sel_bits(ukey));
        double s0[8], s1[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = 8 * tid + e;                          // y_{j+1}
            s0[e] = 0.0;
            s1[e] = 0.0;
            if (j < k) {
                const double y = __longlong_as_double((long long)sel_bits(keys[j])) - uval;
                s0[e] = y;
                s1[e] = (double)(k - (j + 1)) * y;
            }
        }
        double t0 = ((s0[0] + s0[1]) + (s0[2] + s0[3])) + ((s0[4] + s0[5]) + (s0[6] + s0[7]));
        double t1 = ((s1[0] + s1[1]) + (s1[2] + s1[3])) + ((s1[4] + s1[5]) + (s1[6] + s1[7]));
        for (int o = 1; o < 64; o <<= 1) {
            t0 = t0 + __shfl_xor(t0, o, 64);
            t1 = t1 + __shfl_xor(t1, o, 64);
        }
        if (lane == 0) { part[0][wave] = t0; part[1][wave] = t1; }
        __syncthreads();
        if (tid < 64) {
            const double S0 = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
            const double S1 = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
            const double a0 = S0 / (double)k;
            const double a1 = S1 / ((double)k * (double)(k - 1));
            const double d = a0 - 2.0 * a1;
            const bool ok = d > 0.0 && a1 > 0.0;
            const double xi = 2.0 - a0 / d;
            const double sigma = ((2.0 * a0) * a1) / d;
            if (tid == 0) {
                param[0] = sel_bits(ukey);
                param[1] = ok ? (uint64_t)__double_as_longlong(xi) : kSelNaN;
                param[2] = ok ? (uint64_t)__double_as_longlong(sigma) : kSelNaN;
            }
            if (tid < a.n_period) {
                const double L = a.L[tid];
                uint64_t out = kSelNaN;
                if (ok && L >= 0.0) {
                    const double lv = xi == 0.0 ? uval + sigma * L : uval + sigma * expm1(xi * L) / xi;
                    out = (uint64_t)__double_as_longlong(lv);
                }
                level[tid] = out;
            }
        }
        __syncthreads();
    }
}

int tail_check(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, int32_t k, double total_years,
               int32_t n_period, const double *periods, const double *param, const double *level)
{
    if (!periods || !param || !level || (n_row > 0 && !plane)) return fail(ctx, "tcr_tail: NULL argument");
    if (n_row < 0) return fail(ctx, "tcr_tail: n_row must be >= 0");
    if (n_col < 1 || n_col > INT32_MAX) return fail(ctx, "tcr_tail: n_col must be in [1, 2^31 - 1]");
    if (row_stride < n_col) return fail(ctx, "tcr_tail: row_stride must be >= n_col");
    if (n_row > 1 && row_stride > INT64_MAX / (8 * n_row)) return fail(ctx, "tcr_tail: the plane is too large");
    if (k < 2 || k > TCR_TAIL_MAX_K) return fail(ctx, "tcr_tail: k must be in [2, 2048]");
    if (!(std::isfinite(total_years) && total_years > 0.0)) return fail(ctx, "tcr_tail: total_years must be finite and > 0");
    if (n_period < 1 || n_period > TCR_SELECT_MAX_RANKS) return fail(ctx, "tcr_tail: n_period must be in [1, 64]");
    for (int j = 0; j < n_period; ++j)
        if (!(std::isfinite(periods[j]) && periods[j] > 0.0)) return fail(ctx, "tcr_tail: periods must be finite and > 0");
    return 0;
}

}  // namespace

extern "C" {

int tcr_tail_dev(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, int32_t k, double total_years,
                 int32_t n_period, const double *periods, double *param, double *level, int32_t *n_valid, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || tail_check(ctx, plane, n_row, n_col, row_stride, k, total_years, n_period, periods, param, level)) return -1;
    if (n_row == 0) return 0;
    TailArgs a{};
    a.plane = plane; a.n_row = n_row; a.n_col = n_col; a.stride = row_stride; a.param = param; a.level = level; a.n_valid = n_valid;
    a.k = k; a.n_period = n_period;
    for (int j = 0; j < n_period; ++j) a.L[j] = std::log(((double)k / total_years) * periods[j]);
    hipLaunchKernelGGL(k_row_tail, dim3((unsigned)std::min(n_row, kSelBlocksMax)), dim3(kSelThreads), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int tcr_tail_host(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, int32_t k, double total_years,
                  int32_t n_period, const double *periods, double *param, double *level, int32_t *n_valid)
{
    if (!enter(ctx) || tail_check(ctx, plane, n_row, n_col, row_stride, k, total_years, n_period, periods, param, level)) return -1;
    if (n_row == 0) return 0;
    DevBuf B;
    const size_t n_in = (size_t)(n_row - 1) * (size_t)row_stride + (size_t)n_col, n_out = (size_t)n_row * (size_t)n_period;
    const double *d_plane = B.put(plane, n_in);
    double *d_param = B.get<double>(3 * (size_t)n_row);
    double *d_level = B.get<double>(n_out);
    int32_t *d_valid = B.get<int32_t>((size_t)n_row);
    if (!d_plane || !d_param || !d_level || !d_valid) return fail(ctx, "tcr_tail_host: device allocation / upload failed");
    if (tcr_tail_dev(ctx, d_plane, n_row, n_col, row_stride, k, total_years, n_period, periods, d_param, d_level, d_valid, ctx->stream))
        return -1;
    HIPCHK(ctx, hipMemcpyAsync(param, d_param, sizeof(double) * 3 * (size_t)n_row, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(level, d_level, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
    if (n_valid) HIPCHK(ctx, hipMemcpyAsync(n_valid, d_valid, sizeof(int32_t) * (size_t)n_row, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
