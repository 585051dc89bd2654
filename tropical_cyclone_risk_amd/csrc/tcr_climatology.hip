// Track climatology behind the C ABI (include/tcrisk_hip.h, "track climatology" section): per cell of a lon / lat grid and per
// group of storms, the storms through the cell, those whose in-cell maximum reaches each threshold, genesis and lifetime-maximum
// (LMI) counts and the fixed-point PDI; per storm, its genesis sample, LMI and PDI.
//
// k_climatology: one wave per storm, the storm's samples in chunks of 64 lanes.  Every lane takes one sample: its cell by the
// contract's arithmetic, its q(v), and a running (max, first index) of vmax; a ballot of "live" gives the first live sample.
// The (cell << 32 | k) keys of the live samples inside the grid are compacted (mbcnt) into the wave's slice of LDS (tracks of
// more than kClLds samples: a slice of a context workspace in global memory) and sorted by a bitonic network over the padded
// length, so each cell's samples form one run.  A segmented scan over the sorted keys (shuffles, with the run that continues
// into the next chunk carried) gives every run its vmax max and q sum at its last element, which does the atomics: +1 to
// track, the q sum to pdi, +1 to one bin of a per-cell "max-bin" histogram (the number of thresholds <= the run's max, kept in
// the exceed plane).  k_clim_exceed turns that histogram into exceedance counts by a suffix sum over the bins.  Each
// (storm, cell) pair costs two or three integer atomics, whatever the number of thresholds.  Every output is an integer sum or
// a copy of an input, so results are bit-identical from run to run and independent of the launch shape and storm order.

namespace {

constexpr int kClWaves = 4;                 // storms (waves) per block
constexpr int kClLds = 512;                 // keys of one storm in LDS (4 KB per wave); longer tracks sort in the workspace
constexpr int kClMaxBin = 64;
constexpr int64_t kClBlocksMax = 16384;
constexpr size_t kClWsBytes = (size_t)256 << 20;   // workspace budget: fewer waves in flight for very long tracks
constexpr uint64_t kClNone = ~0ull;         // padding key: sorts after every (cell, k)

struct ClArgs {
    const double *lon, *lat, *vmax;
    const int32_t *group;
    int64_t n_trk, n_t, stride;
    int32_t n_group, n_bin;
    double lon0, dlon, lat0, dlat;
    int32_t nlon, nlat, global;
    int64_t n_cell;
    tcr_clim_out out;
    uint64_t *ws;                           // [waves][ws_len] (workspace path)
    int64_t ws_len;
    double thr[kClMaxBin];
};

// A wave's lanes read each other's key slots (LDS or the workspace): the slots written before are complete and visible after
// this (workgroup-scope fences: the waits for the wave's own LDS / vector-memory counters, no cache maintenance)
__device__ __forceinline__ void cl_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the contract's cell of a live sample, -1 outside the grid
__device__ __forceinline__ int cl_cell(const ClArgs &a, double x, double y)
{
    double t = fmod(x - a.lon0, 360.0);
    if (t < 0.0) t += 360.0;
    if (t >= 360.0) t = 0.0;                // a reduction that rounds up to the period
    if (!(t >= 0.0)) return -1;             // x infinite
    double fi = floor(t / a.dlon);
    if (fi >= (double)a.nlon) {
        if (!a.global) return -1;
        fi = (double)(a.nlon - 1);
    }
    const double fj = floor((y - a.lat0) / a.dlat);
    if (!(fj >= 0.0 && fj < (double)a.nlat)) return -1;
    return (int)fj * a.nlon + (int)fi;
}

__device__ __forceinline__ int64_t cl_q(double v)
{
    if (!(v >= 0.0 && v <= 400.0)) return 0;
    return (int64_t)rint(((v * v) * v) * 1024.0);
}

__device__ __forceinline__ int cl_lanes_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

template <bool kLds>
__global__ __launch_bounds__(64 * kClWaves) void k_climatology(ClArgs a)
{
    __shared__ uint64_t cl_lds[kLds ? kClWaves * kClLds : 1];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t wave0 = (int64_t)blockIdx.x * kClWaves + wid, n_waves = (int64_t)gridDim.x * kClWaves;
    uint64_t *keys = kLds ? cl_lds + wid * kClLds : a.ws + wave0 * a.ws_len;
    for (int64_t s = wave0; s < a.n_trk; s += n_waves) {
        const double *lon = a.lon + s * a.stride, *lat = a.lat + s * a.stride, *vm = a.vmax + s * a.stride;
        const int32_t g = a.group[s];
        const bool mapped = g >= 0 && g < a.n_group;
        int first_k = -1, first_cell = -1;          // wave-uniform
        int best_k = -1, best_cell = -1;            // per lane: the first of its samples attaining its max of vmax
        double best_v = NAN;
        int64_t qs = 0;
        int n_key = 0;                              // wave-uniform
        for (int64_t k0 = 0; k0 < a.n_t; k0 += 64) {
            const int k = (int)k0 + lane;
            double x = NAN, y = NAN, v = NAN;
            if (k < a.n_t) { x = lon[k]; y = lat[k]; v = vm[k]; }
            const bool live = !isnan(x) && !isnan(y);
            const int cell = live ? cl_cell(a, x, y) : -1;
            const unsigned long long L = __ballot(live);
            if (first_k < 0 && L) {
                const int q = __builtin_ctzll(L);
                first_k = (int)k0 + q;
                first_cell = __shfl(cell, q);
            }
            if (live) {
                qs += cl_q(v);
                if (!isnan(v) && (best_k < 0 || v > best_v)) { best_v = v; best_k = k; best_cell = cell; }
            }
            const unsigned long long I = __ballot(cell >= 0);
            if (cell >= 0) keys[n_key + cl_lanes_below(I)] = ((uint64_t)(uint32_t)cell << 32) | (uint32_t)k;
            n_key += __popcll(I);
        }
        // the storm's LMI (largest v, then lowest k) and PDI over the wave
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best_v, off);
            const int ok = __shfl_xor(best_k, off), oc = __shfl_xor(best_cell, off);
            qs += __shfl_xor(qs, off);
            if (ok >= 0 && (best_k < 0 || ov > best_v || (ov == best_v && ok < best_k))) { best_v = ov; best_k = ok; best_cell = oc; }
        }
        if (lane == 0) {
            a.out.genesis_k[s] = first_k;
            a.out.lmi_v[s] = best_k >= 0 ? best_v : NAN;
            a.out.lmi_k[s] = best_k;
            a.out.pdi_storm[s] = qs;
            if (mapped && first_cell >= 0) atomicAdd(a.out.genesis + g * a.n_cell + first_cell, 1);
            if (mapped && best_cell >= 0) atomicAdd(a.out.lmi + g * a.n_cell + best_cell, 1);
        }
        if (!mapped || n_key == 0) continue;

        // bitonic sort of the keys, padded to a power of two
        int P = 1;
        while (P < n_key) P <<= 1;
        for (int e = n_key + lane; e < P; e += 64) keys[e] = kClNone;
        cl_wave_sync();
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = lane; t < (P >> 1); t += 64) {
                    const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                    const uint64_t u = keys[i], w = keys[j];
                    if ((u > w) == ((i & size) == 0)) { keys[i] = w; keys[j] = u; }
                }
                cl_wave_sync();
            }

        // runs of one cell: segmented (max v, sum q) scan, the run's last element does the atomics
        double c_v = NAN;                           // the run that continues from the previous chunk
        int64_t c_q = 0;
        for (int e0 = 0; e0 < n_key; e0 += 64) {
            const int e = e0 + lane;
            const bool ok = e < n_key;
            const uint64_t key = ok ? keys[e] : kClNone;
            const uint32_t cell = (uint32_t)(key >> 32);
            bool f = ok && (e == 0 || (uint32_t)(keys[e - 1] >> 32) != cell);            // run head
            const bool tail = ok && (e + 1 == n_key || (uint32_t)(keys[e + 1] >> 32) != cell);
            double v = NAN;
            int64_t q = 0;
            if (ok) {
                v = vm[(uint32_t)key];
                q = cl_q(v);
            }
            for (int off = 1; off < 64; off <<= 1) {
                const double ov = __shfl_up(v, off);
                const int64_t oq = __shfl_up(q, off);
                const bool of = __shfl_up((int)f, off) != 0;
                if (lane >= off && !f) { v = fmax(v, ov); q += oq; f = of; }
            }
            if (ok && !f) { v = fmax(v, c_v); q += c_q; }     // no head in this chunk before me: the carried run
            if (tail) {
                const int64_t at = (int64_t)g * a.n_cell + cell;
                atomicAdd(a.out.track + at, 1);
                if (q) atomicAdd(reinterpret_cast<unsigned long long *>(a.out.pdi + at), (unsigned long long)q);
                int c = 0;
                for (int b = 0; b < a.n_bin; ++b) c += a.thr[b] <= v;                       // NaN: 0
                if (c) atomicAdd(a.out.exceed + ((int64_t)g * a.n_bin + c - 1) * a.n_cell + cell, 1);
            }
            c_v = __shfl(v, 63);
            c_q = __shfl(q, 63);
        }
        cl_wave_sync();                             // the next storm overwrites the keys
    }
}

// exceed[g][b][cell] <- sum over b' >= b of the max-bin histogram (storms whose in-cell max reaches thresholds[b])
__global__ __launch_bounds__(256) void k_clim_exceed(int32_t *exceed, int64_t n_group, int32_t n_bin, int64_t n_cell)
{
    const int64_t n = n_group * n_cell;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = i / n_cell;
        int32_t *p = exceed + g * n_bin * n_cell + (i - g * n_cell);
        int32_t run = 0;
        for (int b = n_bin - 1; b >= 0; --b) {
            run += p[b * n_cell];
            p[b * n_cell] = run;
        }
    }
}

int clim_check(tcr_ctx *ctx, const tcr_hazard_tracks *t, const int32_t *group, int32_t n_group, const tcr_clim_grid *gr,
               int32_t n_bin, const double *thr, const tcr_clim_out *o)
{
    if (!t || !gr || !o) return fail(ctx, "tcr_climatology: NULL argument");
    if (t->n_trk < 0 || t->n_t < 1 || t->row_stride < t->n_t || t->n_t > ((int64_t)1 << 27) ||
        t->n_trk > (((int64_t)1 << 27) / t->n_t))
        return fail(ctx, "tcr_climatology: bad sizes (n_trk >= 0, 1 <= n_t, row_stride >= n_t, n_trk * n_t <= 2^27)");
    const bool fin = std::isfinite(gr->lon0) && std::isfinite(gr->dlon) && std::isfinite(gr->lat0) && std::isfinite(gr->dlat);
    if (!fin || !(gr->dlon > 0.0) || !(gr->dlat > 0.0) || gr->nlon < 1 || gr->nlat < 1 || gr->nlon > ((int64_t)1 << 31) ||
        !((double)gr->nlon * gr->dlon <= 360.0) || gr->nlat >= (((int64_t)1 << 31) + gr->nlon - 1) / gr->nlon)
        return fail(ctx, "tcr_climatology: bad grid (finite; dlon, dlat > 0; nlon, nlat >= 1; nlon * dlon <= 360; "
                         "nlon * nlat < 2^31)");
    if (n_group < 1) return fail(ctx, "tcr_climatology: n_group must be >= 1");
    if (n_bin < 0 || n_bin > kClMaxBin) return fail(ctx, "tcr_climatology: n_bin must be in [0, 64]");
    if ((double)n_group * (double)(gr->nlon * gr->nlat) * (double)(n_bin > 0 ? n_bin : 1) > 9.0e15)
        return fail(ctx, "tcr_climatology: n_group x cells x bins too large");
    if (n_bin > 0 && !thr) return fail(ctx, "tcr_climatology: NULL thresholds");
    for (int b = 0; b < n_bin; ++b)
        if (!std::isfinite(thr[b]) || (b > 0 && !(thr[b] > thr[b - 1])))
            return fail(ctx, "tcr_climatology: thresholds must be finite and strictly ascending");
    if (!o->track || !o->genesis || !o->lmi || !o->pdi || (n_bin > 0 && !o->exceed))
        return fail(ctx, "tcr_climatology: NULL map");
    if (t->n_trk > 0 && (!t->lon || !t->lat || !t->vmax || !group)) return fail(ctx, "tcr_climatology: NULL track plane or group");
    if (t->n_trk > 0 && (!o->genesis_k || !o->lmi_v || !o->lmi_k || !o->pdi_storm))
        return fail(ctx, "tcr_climatology: NULL per-storm output");
    return 0;
}

}  // namespace

extern "C" {

int tcr_climatology_dev(tcr_ctx *ctx, const tcr_hazard_tracks *t, const int32_t *group, int32_t n_group, const tcr_clim_grid *gr,
                        int32_t n_bin, const double *thresholds, const tcr_clim_out *o, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || clim_check(ctx, t, group, n_group, gr, n_bin, thresholds, o)) return -1;
    const int64_t n_cell = gr->nlon * gr->nlat, n_map = (int64_t)n_group * n_cell;
    HIPCHK(ctx, hipMemsetAsync(o->track, 0, sizeof(int32_t) * n_map, st));
    HIPCHK(ctx, hipMemsetAsync(o->genesis, 0, sizeof(int32_t) * n_map, st));
    HIPCHK(ctx, hipMemsetAsync(o->lmi, 0, sizeof(int32_t) * n_map, st));
    HIPCHK(ctx, hipMemsetAsync(o->pdi, 0, sizeof(int64_t) * n_map, st));
    if (n_bin > 0) HIPCHK(ctx, hipMemsetAsync(o->exceed, 0, sizeof(int32_t) * n_map * n_bin, st));
    if (t->n_trk == 0) return 0;
    ClArgs a{};
    a.lon = t->lon; a.lat = t->lat; a.vmax = t->vmax; a.group = group;
    a.n_trk = t->n_trk; a.n_t = t->n_t; a.stride = t->row_stride;
    a.n_group = n_group; a.n_bin = n_bin;
    a.lon0 = gr->lon0; a.dlon = gr->dlon; a.lat0 = gr->lat0; a.dlat = gr->dlat;
    a.nlon = (int32_t)gr->nlon; a.nlat = (int32_t)gr->nlat;
    a.global = (double)gr->nlon * gr->dlon == 360.0;
    a.n_cell = n_cell;
    a.out = *o;
    for (int b = 0; b < n_bin; ++b) a.thr[b] = thresholds[b];
    int64_t blocks = std::min<int64_t>(kClBlocksMax, (t->n_trk + kClWaves - 1) / kClWaves);
    if (t->n_t <= kClLds) {
        hipLaunchKernelGGL(k_climatology<true>, dim3((unsigned)blocks), dim3(64 * kClWaves), 0, st, a);
    } else {
        int64_t P = 1;
        while (P < t->n_t) P <<= 1;
        const int64_t waves = std::max<int64_t>(1, std::min<int64_t>(blocks * kClWaves, (int64_t)(kClWsBytes / (sizeof(uint64_t) * P))));
        blocks = (waves + kClWaves - 1) / kClWaves;
        const size_t bytes = sizeof(uint64_t) * (size_t)P * (size_t)std::min<int64_t>(t->n_trk, blocks * kClWaves);   // waves with a storm
        if (ctx->an.d_cl.grow(ctx, bytes / sizeof(uint64_t)) < 0) return -1;
        a.ws = ctx->an.d_cl.p;
        a.ws_len = P;
        hipLaunchKernelGGL(k_climatology<false>, dim3((unsigned)blocks), dim3(64 * kClWaves), 0, st, a);
    }
    HIPCHK(ctx, hipGetLastError());
    if (n_bin > 1) {
        const unsigned eb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (n_map + 255) / 256));
        hipLaunchKernelGGL(k_clim_exceed, dim3(eb), dim3(256), 0, st, o->exceed, (int64_t)n_group, n_bin, n_cell);
        HIPCHK(ctx, hipGetLastError());
    }
    return 0;
}

int tcr_climatology_host(tcr_ctx *ctx, const tcr_hazard_tracks *t, const int32_t *group, int32_t n_group, const tcr_clim_grid *gr,
                         int32_t n_bin, const double *thresholds, const tcr_clim_out *o)
{
    if (!enter(ctx) || clim_check(ctx, t, group, n_group, gr, n_bin, thresholds, o)) return -1;
    DevBuf B;
    const size_t n_trk = (size_t)t->n_trk;
    const size_t n_map = (size_t)n_group * (size_t)(gr->nlon * gr->nlat), n_ex = n_map * (size_t)n_bin;
    tcr_hazard_tracks d;
    const int32_t *d_group = B.put(group, n_trk);
    tcr_clim_out dout{};
    dout.track = B.get<int32_t>(n_map); dout.genesis = B.get<int32_t>(n_map); dout.lmi = B.get<int32_t>(n_map);
    dout.pdi = B.get<int64_t>(n_map);
    dout.exceed = n_bin > 0 ? B.get<int32_t>(n_ex) : nullptr;
    dout.genesis_k = B.get<int32_t>(n_trk); dout.lmi_v = B.get<double>(n_trk); dout.lmi_k = B.get<int32_t>(n_trk);
    dout.pdi_storm = B.get<int64_t>(n_trk);
    const bool ok = hazard_tracks_upload(B, t, &d) && d_group && dout.track && dout.genesis && dout.lmi && dout.pdi &&
                    (n_bin == 0 || dout.exceed) && dout.genesis_k && dout.lmi_v && dout.lmi_k && dout.pdi_storm;
    if (!ok) return fail(ctx, "tcr_climatology_host: device allocation / upload failed");
    if (tcr_climatology_dev(ctx, &d, d_group, n_group, gr, n_bin, thresholds, &dout, ctx->stream)) return -1;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(o->track, dout.track, sizeof(int32_t) * n_map, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(o->genesis, dout.genesis, sizeof(int32_t) * n_map, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(o->lmi, dout.lmi, sizeof(int32_t) * n_map, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(o->pdi, dout.pdi, sizeof(int64_t) * n_map, hipMemcpyDeviceToHost, st));
    if (n_bin > 0) HIPCHK(ctx, hipMemcpyAsync(o->exceed, dout.exceed, sizeof(int32_t) * n_ex, hipMemcpyDeviceToHost, st));
    if (n_trk) {
        HIPCHK(ctx, hipMemcpyAsync(o->genesis_k, dout.genesis_k, sizeof(int32_t) * n_trk, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(o->lmi_v, dout.lmi_v, sizeof(double) * n_trk, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(o->lmi_k, dout.lmi_k, sizeof(int32_t) * n_trk, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(o->pdi_storm, dout.pdi_storm, sizeof(int64_t) * n_trk, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
