// Row packing behind the C ABI (include/tcrisk_hip.h, "row packing (event footprints)" section): the entries of every row of a
// [n_row][n_col] plane that are >= a floor, in ascending column order, as CSR (row_ptr, col, val).  It is what turns the per-storm
// plane of a site analysis (site_max, site_total, ...) into the event table of a block of sites while the plane is on the device.
//
//   k_rowpack_count   one 256-thread workgroup per row (several rows in turn past kPackBlocksMax).  A turn of the workgroup covers
//                     kPackTurn = 256 x kPackUnroll columns: wave w takes the kPackUnroll runs of 64 columns from w x 64 x
//                     kPackUnroll on, so a lane has kPackUnroll loads in flight and every load of a wave is 512 adjacent bytes.
//                     Kept entries are counted by ballot + popcount; the four wave totals meet in LDS and one int64 goes to
//                     row_ptr[r + 1];
//   k_rowpack_scan    one workgroup: the inclusive sum over row_ptr[1 ..] in place, and row_ptr[0] = 0 (integer sums: any shape of
//                     the scan gives the same bits);
//   k_rowpack_fill    the sweep of k_rowpack_count again.  Columns ascend with (turn, wave, run, lane), so the position of a kept
//                     entry is the row's start + the kept entries of the earlier turns + the totals of the lower waves of this turn
//                     (four wave totals through LDS, one barrier per turn: the totals alternate between two LDS slots) + the lower
//                     runs of its wave + popcount(ballot & lanes below).  No atomics: a position is a function of the plane.  Every
//                     wave makes every turn of a row, whatever it holds: the barrier and the ballots need all of them.  Positions
//                     are 64-bit, and an entry at or past `capacity` (or before 0) is dropped, whatever row_ptr says.
//
// A value is kept iff value >= min_value as an IEEE comparison (a NaN never is; -0.0 >= 0.0 is); val is a bit copy of it.

namespace {

constexpr int kPackThreads = 256;
constexpr int kPackWaves = kPackThreads / 64;
constexpr int kPackUnroll = TCR_ROWPACK_UNROLL;         // loads a lane has in flight
constexpr int kPackSpan = 64 * kPackUnroll;             // adjacent columns of one wave in a turn
constexpr int kPackTurn = kPackThreads * kPackUnroll;   // columns of one turn of the workgroup
constexpr int64_t kPackBlocksMax = 1 << 16;             // more rows than this: a workgroup takes several, one after the other
constexpr int kPackScanItems = 16;                      // adjacent row counts a thread of k_rowpack_scan sums
constexpr uint64_t kPackNaN = 0x7ff8000000000000ull;

__device__ __forceinline__ bool pack_keep(uint64_t bits, double floor) { return __longlong_as_double((long long)bits) >= floor; }

__global__ __launch_bounds__(kPackThreads) void k_rowpack_count(const double *plane, int64_t n_row, int64_t n_col, int64_t stride,
                                                                double floor, int64_t *row_ptr)
{
    __shared__ int64_t tot[2][kPackWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int par = 0;
    for (int64_t r = blockIdx.x; r < n_row; r += gridDim.x) {
        const uint64_t *row = reinterpret_cast<const uint64_t *>(plane) + r * stride;
        int64_t n = 0;                                      // (the same on every lane of the wave)
        for (int64_t base = (int64_t)wave * kPackSpan; base < n_col; base += kPackTurn) {
            uint64_t bits[kPackUnroll];
#pragma unroll
            for (int u = 0; u < kPackUnroll; ++u) {
                const int64_t i = base + u * 64 + lane;
                bits[u] = i < n_col ? row[i] : kPackNaN;
            }
#pragma unroll
            for (int u = 0; u < kPackUnroll; ++u) n += __popcll(__ballot(pack_keep(bits[u], floor)));
        }
        // (slot par was last read two rows ago, before the barrier of the row in between)
        if (lane == 0) tot[par][wave] = n;
        __syncthreads();
        if (tid == 0) row_ptr[r + 1] = tot[par][0] + tot[par][1] + tot[par][2] + tot[par][3];
        par ^= 1;
    }
}

// row_ptr[1 .. n_row] <- its inclusive sums, row_ptr[0] <- 0.  One workgroup; a thread sums kPackScanItems adjacent counts.
__global__ __launch_bounds__(kPackThreads) void k_rowpack_scan(int64_t *row_ptr, int64_t n_row)
{
    __shared__ int64_t wsum[kPackWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t *c = row_ptr + 1;
    int64_t carry = 0;
    for (int64_t t0 = 0; t0 < n_row; t0 += (int64_t)kPackThreads * kPackScanItems) {
        const int64_t i0 = t0 + (int64_t)tid * kPackScanItems;
        int64_t v[kPackScanItems];
        int64_t sum = 0;
#pragma unroll
        for (int k = 0; k < kPackScanItems; ++k) {
            sum += i0 + k < n_row ? c[i0 + k] : 0;
            v[k] = sum;
        }
        int64_t inc = sum;                                  // inclusive over the lanes of the wave
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t x = __shfl_up(inc, o, 64);
            if (lane >= o) inc += x;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int64_t off = carry + (inc - sum), all = 0;
#pragma unroll
        for (int w = 0; w < kPackWaves; ++w) {
            const int64_t t = wsum[w];
            off += w < wave ? t : 0;
            all += t;
        }
        carry += all;
        __syncthreads();                                    // (wsum is written again in the next tile)
#pragma unroll
        for (int k = 0; k < kPackScanItems; ++k)
            if (i0 + k < n_row) c[i0 + k] = off + v[k];
    }
    if (tid == 0) row_ptr[0] = 0;
}

__global__ __launch_bounds__(kPackThreads) void k_rowpack_fill(const double *plane, int64_t n_row, int64_t n_col, int64_t stride,
                                                               double floor, const int64_t *row_ptr, int64_t capacity, int32_t *col,
                                                               double *val)
{
    __shared__ int32_t tot[2][kPackWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint64_t *out = reinterpret_cast<uint64_t *>(val);
    int par = 0;
    for (int64_t r = blockIdx.x; r < n_row; r += gridDim.x) {
        const uint64_t *row = reinterpret_cast<const uint64_t *>(plane) + r * stride;
        int64_t at = row_ptr[r];                            // the row's start + the kept entries of the earlier turns
        for (int64_t t0 = 0; t0 < n_col; t0 += kPackTurn) { // (the same turns on every wave)
            const int64_t base = t0 + (int64_t)wave * kPackSpan;
            uint64_t bits[kPackUnroll];
            unsigned long long m[kPackUnroll];
#pragma unroll
            for (int u = 0; u < kPackUnroll; ++u) {
                const int64_t i = base + u * 64 + lane;
                bits[u] = i < n_col ? row[i] : kPackNaN;
            }
            int wn = 0;
#pragma unroll
            for (int u = 0; u < kPackUnroll; ++u) {
                m[u] = __ballot(pack_keep(bits[u], floor));
                wn += __popcll(m[u]);
            }
            // (slot par was last read two turns ago, before the barrier of the turn in between)
            if (lane == 0) tot[par][wave] = wn;
            __syncthreads();
            int64_t pos = at;
#pragma unroll
            for (int w = 0; w < kPackWaves; ++w) {
                const int32_t t = tot[par][w];
                pos += w < wave ? t : 0;
                at += t;
            }
            par ^= 1;
#pragma unroll
            for (int u = 0; u < kPackUnroll; ++u) {
                const int64_t p = pos + __popcll(m[u] & below);
                if (((m[u] >> lane) & 1ull) && (uint64_t)p < (uint64_t)capacity) {
                    col[p] = (int32_t)(base + u * 64 + lane);
                    out[p] = bits[u];
                }
                pos += __popcll(m[u]);
            }
        }
    }
}

int rowpack_check(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, double min_value,
                  const int64_t *row_ptr, int64_t capacity)
{
    if (!row_ptr || (n_row > 0 && !plane)) return fail(ctx, "tcr_rowpack: NULL argument");
    if (n_row < 0) return fail(ctx, "tcr_rowpack: n_row must be >= 0");
    if (n_col < 1 || n_col > INT32_MAX) return fail(ctx, "tcr_rowpack: n_col must be in [1, 2^31 - 1]");
    if (row_stride < n_col) return fail(ctx, "tcr_rowpack: row_stride must be >= n_col");
    if (n_row > 1 && row_stride > INT64_MAX / (8 * n_row)) return fail(ctx, "tcr_rowpack: the plane is too large");
    if (min_value != min_value) return fail(ctx, "tcr_rowpack: min_value must not be NaN");
    if (capacity < 0) return fail(ctx, "tcr_rowpack: capacity must be >= 0");
    return 0;
}

}  // namespace

extern "C" {

int tcr_rowpack_count_dev(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, double min_value,
                          int64_t *row_ptr, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || rowpack_check(ctx, plane, n_row, n_col, row_stride, min_value, row_ptr, 0)) return -1;
    if (n_row == 0) {
        HIPCHK(ctx, hipMemsetAsync(row_ptr, 0, sizeof(int64_t), st));
        return 0;
    }
    hipLaunchKernelGGL(k_rowpack_count, dim3((unsigned)std::min(n_row, kPackBlocksMax)), dim3(kPackThreads), 0, st, plane, n_row, n_col,
                       row_stride, min_value, row_ptr);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_rowpack_scan, dim3(1), dim3(kPackThreads), 0, st, row_ptr, n_row);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int tcr_rowpack_fill_dev(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, double min_value,
                         const int64_t *row_ptr, int64_t capacity, int32_t *col, double *val, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || rowpack_check(ctx, plane, n_row, n_col, row_stride, min_value, row_ptr, capacity)) return -1;
    if (capacity > 0 && (!col || !val)) return fail(ctx, "tcr_rowpack: NULL argument");
    if (n_row == 0 || capacity == 0) return 0;
    hipLaunchKernelGGL(k_rowpack_fill, dim3((unsigned)std::min(n_row, kPackBlocksMax)), dim3(kPackThreads), 0, st, plane, n_row, n_col,
                       row_stride, min_value, row_ptr, capacity, col, val);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int tcr_rowpack_host(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, double min_value,
                     int64_t *row_ptr, int64_t capacity, int32_t *col, double *val)
{
    if (!enter(ctx) || rowpack_check(ctx, plane, n_row, n_col, row_stride, min_value, row_ptr, capacity)) return -1;
    const bool count_only = capacity == 0 && !col && !val;
    if (!count_only && (!col || !val)) return fail(ctx, "tcr_rowpack: NULL argument");
    if (n_row == 0) {
        row_ptr[0] = 0;
        return 0;
    }
    DevBuf B;
    const size_t n_in = (size_t)(n_row - 1) * (size_t)row_stride + (size_t)n_col;
    const double *d_plane = B.put(plane, n_in);
    int64_t *d_ptr = B.get<int64_t>((size_t)n_row + 1);
    if (!d_plane || !d_ptr) return fail(ctx, "tcr_rowpack: device allocation / upload failed");
    if (tcr_rowpack_count_dev(ctx, d_plane, n_row, n_col, row_stride, min_value, d_ptr, ctx->stream)) return -1;
    HIPCHK(ctx, copy_sync(ctx->stream, row_ptr, d_ptr, sizeof(int64_t) * ((size_t)n_row + 1), hipMemcpyDeviceToHost));
    const int64_t nnz = row_ptr[n_row];
    if (count_only) return 0;
    if (nnz > capacity) return fail(ctx, "tcr_rowpack: capacity is smaller than the number of kept entries (row_ptr[n_row])");
    if (nnz == 0) return 0;
    int32_t *d_col = B.get<int32_t>((size_t)nnz);
    double *d_val = B.get<double>((size_t)nnz);
    if (!d_col || !d_val) return fail(ctx, "tcr_rowpack: device allocation / upload failed");
    if (tcr_rowpack_fill_dev(ctx, d_plane, n_row, n_col, row_stride, min_value, d_ptr, nnz, d_col, d_val, ctx->stream)) return -1;
    HIPCHK(ctx, hipMemcpyAsync(col, d_col, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(val, d_val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
