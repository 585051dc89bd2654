// Landfall detection behind the C ABI (include/tcrisk_hip.h, "landfall" section): where the model's own land decision sees a
// storm go from sea to land, and how strong it was there.
//
// The land decision.  The model is over land where the bilinear interpolant of the land grid equals 1
// (coupled_fast.py:35-38).  Here the same decision is taken on the nodes, without arithmetic: a node is land iff land >= 1 (NaN:
// water); a sample is over land iff every node with a nonzero bilinear weight is land.  The sample's cell is found by comparisons
// against the node coordinates (i = the last node <= x, 0 below the grid; node i + 1 has a nonzero weight iff it exists and
// lon_i < x), so the bilinear sum's rounding (the ~1.5 % flicker of `== 1` inside land) does not enter.  A periodic grid
// (lon[n-1] - lon[0] + (lon[1] - lon[0]) == 360) reduces x into [lon0, lon0 + 360) first, and its last cell wraps to node 0.
//
// One kernel, k_landfall: one wave per storm, the storm's samples in chunks of 64 lanes.  Every lane takes one sample's land
// decision; ballots of "live" (lon, lat not NaN) and "over land", with the last live sample of the previous chunks carried in
// scalars, give each lane its previous live sample, so a sea -> land step is found without a serial walk.  mbcnt over the ballot of
// events gives each event its slot.  The node coordinates sit in LDS (copied once per block; a grid too large for it reads them
// from global memory), the land nodes are a bit plane (0.5 MB for the 0.125-degree globe: it stays in L2).  The cell guess from the
// mean spacing only decides where the comparisons start.  Every output is a copy of an input or an integer, so results are
// bit-identical from run to run and independent of the launch shape.

namespace {

constexpr int kLfWaves = 4;                 // storms (waves) per block
constexpr int kLfLdsMax = 8192;             // node coordinates held in LDS (64 KB); larger grids read them from global memory
constexpr int kLfBlocksMax = 1024;

struct LfGrid {
    const double *xy;                       // [nlon] lon, then [nlat] lat (device)
    const uint32_t *bits;                   // land bit of node (j, i) at j * nlon + i
    int32_t nlon, nlat, periodic;
    double lon0, lon_inv, lat0, lat_inv;    // cell guess (x - x0) * inv
};

struct LfArgs {
    LfGrid g;
    const double *lon, *lat, *vmax;
    int64_t n_trk, n_t, stride;
    int32_t max_events;
    int32_t *n_lf, *ev_k;                   // [n_trk], [n_trk][max_events]
    double *ev_lon, *ev_lat, *ev_v, *ev_vin;
    uint8_t *flags;                         // [n_trk][n_t] or NULL
};

// i = the last node <= x (0 when x is below the grid or NaN); *two: node i + 1 (node 0 across the wrap) has a nonzero weight
__device__ __forceinline__ int lf_cell(const double *xs, int n, double x0, double inv, bool wrap, double x, bool *two)
{
    const double g = fmin(fmax((x - x0) * inv, 0.0), (double)(n - 1));     // fmax drops a NaN: guess 0
    int i = (int)g;
    while (i > 0 && xs[i] > x) --i;
    while (i + 1 < n && xs[i + 1] <= x) ++i;
    *two = (i + 1 < n || wrap) && xs[i] < x;
    return i;
}

__device__ __forceinline__ bool lf_bit(const uint32_t *bits, int64_t node) { return (bits[node >> 5] >> (node & 31)) & 1u; }

__device__ __forceinline__ bool lf_over_land(const LfGrid &g, const double *xs, const double *ys, double x, double y)
{
    if (g.periodic) {
        double t = fmod(x - g.lon0, 360.0);
        if (t < 0.0) t += 360.0;
        x = g.lon0 + t;
        if (x >= g.lon0 + 360.0) x = g.lon0;            // a reduction that rounds up to the period is node 0
    }
    bool tx, ty;
    const int i = lf_cell(xs, g.nlon, g.lon0, g.lon_inv, g.periodic != 0, x, &tx);
    const int j = lf_cell(ys, g.nlat, g.lat0, g.lat_inv, false, y, &ty);
    const int i1 = i + 1 < g.nlon ? i + 1 : 0;
    const int64_t r0 = (int64_t)j * g.nlon, r1 = r0 + g.nlon;
    bool land = lf_bit(g.bits, r0 + i);
    if (tx) land = land && lf_bit(g.bits, r0 + i1);
    if (ty) {
        land = land && lf_bit(g.bits, r1 + i);
        if (tx) land = land && lf_bit(g.bits, r1 + i1);
    }
    return land;
}

__device__ __forceinline__ int lf_lanes_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

template <bool kLds>
__global__ __launch_bounds__(64 * kLfWaves) void k_landfall(LfArgs a)
{
    extern __shared__ double lf_xy[];
    const int n_xy = a.g.nlon + a.g.nlat;
    const double *xy = a.g.xy;
    if (kLds) {
        for (int i = threadIdx.x; i < n_xy; i += 64 * kLfWaves) lf_xy[i] = a.g.xy[i];
        __syncthreads();
        xy = lf_xy;
    }
    const double *xs = xy, *ys = xy + a.g.nlon;
    const int lane = threadIdx.x & 63;
    const unsigned long long below_me = (1ull << lane) - 1ull;
    const int64_t wave0 = (int64_t)blockIdx.x * kLfWaves + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * kLfWaves;
    for (int64_t s = wave0; s < a.n_trk; s += n_waves) {
        const double *lon = a.lon + s * a.stride, *lat = a.lat + s * a.stride, *vm = a.vmax + s * a.stride;
        const int64_t row = s * a.max_events;
        int n_ev = 0;                               // events so far (wave-uniform)
        int64_t prev_k = -1;                        // the last live sample of the previous chunks, and whether it is over land
        bool prev_land = false;
        for (int64_t k0 = 0; k0 < a.n_t; k0 += 64) {
            const int64_t k = k0 + lane;
            double x = NAN, y = NAN;
            if (k < a.n_t) { x = lon[k]; y = lat[k]; }
            const bool live = !isnan(x) && !isnan(y);
            const bool land = live && lf_over_land(a.g, xs, ys, x, y);
            const unsigned long long L = __ballot(live), M = __ballot(land);
            const unsigned long long before = L & below_me;
            int64_t p = prev_k;
            bool p_land = prev_land;
            if (before) {
                const int q = 63 - __clzll(before);
                p = k0 + q;
                p_land = (M >> q) & 1ull;
            }
            const bool ev = land && p >= 0 && !p_land;
            const unsigned long long E = __ballot(ev);
            if (ev) {
                const int pos = n_ev + lf_lanes_below(E);
                if (pos < a.max_events) {
                    a.ev_k[row + pos] = (int32_t)k;
                    a.ev_lon[row + pos] = x;
                    a.ev_lat[row + pos] = y;
                    a.ev_v[row + pos] = vm[p];
                    a.ev_vin[row + pos] = vm[k];
                }
            }
            if (a.flags && k < a.n_t) a.flags[s * a.n_t + k] = live ? (land ? 1 : 0) : 2;
            n_ev += __popcll(E);
            if (L) {
                const int q = 63 - __clzll(L);
                prev_k = k0 + q;
                prev_land = (M >> q) & 1ull;
            }
        }
        for (int e = min(n_ev, a.max_events) + lane; e < a.max_events; e += 64) {      // unused slots: k = -1, NaN
            a.ev_k[row + e] = -1;
            a.ev_lon[row + e] = NAN; a.ev_lat[row + e] = NAN; a.ev_v[row + e] = NAN; a.ev_vin[row + e] = NAN;
        }
        if (lane == 0) a.n_lf[s] = n_ev;
    }
}

int landfall_check(tcr_ctx *ctx, const tcr_hazard_tracks *t, int32_t max_events, const int32_t *n_landfall, const int32_t *ev_k,
                   const double *ev_lon, const double *ev_lat, const double *ev_v, const double *ev_vin)
{
    if (!t || !n_landfall) return fail(ctx, "tcr_landfall: NULL argument");
    if (t->n_trk < 0 || t->n_t < 1 || t->row_stride < t->n_t || t->n_t >= ((int64_t)1 << 31))
        return fail(ctx, "tcr_landfall: bad sizes (n_trk >= 0, 1 <= n_t < 2^31, row_stride >= n_t)");
    if (t->n_trk > 0 && (!t->lon || !t->lat || !t->vmax)) return fail(ctx, "tcr_landfall: NULL track plane");
    if (max_events < 0) return fail(ctx, "tcr_landfall: max_events must be >= 0");
    if (max_events > 0 && (!ev_k || !ev_lon || !ev_lat || !ev_v || !ev_vin)) return fail(ctx, "tcr_landfall: NULL event plane");
    if (!ctx->an.lf_xy.p) return fail(ctx, "tcr_landfall: no land grid on this context (tcr_land_upload)");
    return 0;
}

}  // namespace

extern "C" {

int tcr_land_upload(tcr_ctx *ctx, const tcr_land_grid *grid)
{
    if (!ctx) return -1;
    if (!grid || !grid->lon || !grid->lat || !grid->land) return fail(ctx, "tcr_land_upload: NULL argument");
    const int64_t nlon = grid->nlon, nlat = grid->nlat;
    if (nlon < 2 || nlat < 2 || nlon > ((int64_t)1 << 30) || nlat > ((int64_t)1 << 30) || nlon * nlat > ((int64_t)1 << 36))
        return fail(ctx, "tcr_land_upload: bad sizes (2 <= nlon, nlat; nlon * nlat <= 2^36)");
    for (int64_t i = 0; i < nlon; ++i)
        if (!std::isfinite(grid->lon[i]) || (i > 0 && !(grid->lon[i] > grid->lon[i - 1])))
            return fail(ctx, "tcr_land_upload: lon must be finite and strictly ascending");
    for (int64_t j = 0; j < nlat; ++j)
        if (!std::isfinite(grid->lat[j]) || (j > 0 && !(grid->lat[j] > grid->lat[j - 1])))
            return fail(ctx, "tcr_land_upload: lat must be finite and strictly ascending (flip a north-to-south grid)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t n_node = nlon * nlat, n_word = (n_node + 31) / 32;
    std::vector<uint32_t> bits((size_t)n_word, 0u);
    for (int64_t n = 0; n < n_node; ++n)
        if (grid->land[n] >= 1.0) bits[(size_t)(n >> 5)] |= 1u << (n & 31);
    std::vector<double> xy((size_t)(nlon + nlat));
    memcpy(xy.data(), grid->lon, sizeof(double) * nlon);
    memcpy(xy.data() + nlon, grid->lat, sizeof(double) * nlat);
    // (a new grid starts from nothing: a failure below leaves "no land grid")
    ctx->an.lf_xy.reset(); ctx->an.lf_bits.reset();
    if (ctx->an.lf_xy.upload(ctx, xy.data(), xy.size())) return -1;
    if (ctx->an.lf_bits.upload(ctx, bits.data(), bits.size())) { ctx->an.lf_xy.reset(); return -1; }
    const double *lon = grid->lon, *lat = grid->lat;
    ctx->an.lf_nlon = nlon; ctx->an.lf_nlat = nlat;
    ctx->an.lf_periodic = lon[nlon - 1] - lon[0] + (lon[1] - lon[0]) == 360.0;
    ctx->an.lf_guess[0] = lon[0]; ctx->an.lf_guess[1] = (double)(nlon - 1) / (lon[nlon - 1] - lon[0]);
    ctx->an.lf_guess[2] = lat[0]; ctx->an.lf_guess[3] = (double)(nlat - 1) / (lat[nlat - 1] - lat[0]);
    return 0;
}

int tcr_land_info(tcr_ctx *ctx, int64_t *nlon, int64_t *nlat, int32_t *periodic)
{
    if (!ctx) return -1;
    if (!nlon || !nlat || !periodic) return fail(ctx, "tcr_land_info: NULL argument");
    if (!ctx->an.lf_xy.p) return fail(ctx, "tcr_land_info: no land grid on this context (tcr_land_upload)");
    *nlon = ctx->an.lf_nlon; *nlat = ctx->an.lf_nlat; *periodic = ctx->an.lf_periodic ? 1 : 0;
    return 0;
}

int tcr_landfall_dev(tcr_ctx *ctx, const tcr_hazard_tracks *t, int32_t max_events, int32_t *n_landfall, int32_t *ev_k,
                     double *ev_lon, double *ev_lat, double *ev_v, double *ev_v_inland, uint8_t *flags, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st || landfall_check(ctx, t, max_events, n_landfall, ev_k, ev_lon, ev_lat, ev_v, ev_v_inland)) return -1;
    if (t->n_trk == 0) return 0;
    LfArgs a{};
    a.g.xy = ctx->an.lf_xy.p; a.g.bits = ctx->an.lf_bits.p;
    a.g.nlon = (int32_t)ctx->an.lf_nlon; a.g.nlat = (int32_t)ctx->an.lf_nlat; a.g.periodic = ctx->an.lf_periodic ? 1 : 0;
    a.g.lon0 = ctx->an.lf_guess[0]; a.g.lon_inv = ctx->an.lf_guess[1]; a.g.lat0 = ctx->an.lf_guess[2]; a.g.lat_inv = ctx->an.lf_guess[3];
    a.lon = t->lon; a.lat = t->lat; a.vmax = t->vmax;
    a.n_trk = t->n_trk; a.n_t = t->n_t; a.stride = t->row_stride;
    a.max_events = max_events;
    a.n_lf = n_landfall; a.ev_k = ev_k; a.ev_lon = ev_lon; a.ev_lat = ev_lat; a.ev_v = ev_v; a.ev_vin = ev_v_inland;
    a.flags = flags;
    const unsigned blocks = (unsigned)std::min<int64_t>(kLfBlocksMax, (t->n_trk + kLfWaves - 1) / kLfWaves);
    const int64_t n_xy = ctx->an.lf_nlon + ctx->an.lf_nlat;
    if (n_xy <= kLfLdsMax)
        hipLaunchKernelGGL(k_landfall<true>, dim3(blocks), dim3(64 * kLfWaves), sizeof(double) * n_xy, st, a);
    else
        hipLaunchKernelGGL(k_landfall<false>, dim3(blocks), dim3(64 * kLfWaves), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int tcr_landfall_host(tcr_ctx *ctx, const tcr_hazard_tracks *t, int32_t max_events, int32_t *n_landfall, int32_t *ev_k,
                      double *ev_lon, double *ev_lat, double *ev_v, double *ev_v_inland, uint8_t *flags)
{
    if (!enter(ctx) || landfall_check(ctx, t, max_events, n_landfall, ev_k, ev_lon, ev_lat, ev_v, ev_v_inland)) return -1;
    if (t->n_trk == 0) return 0;
    DevBuf B;
    const size_t n_ev = (size_t)t->n_trk * max_events, n_fl = (size_t)t->n_trk * t->n_t;
    tcr_hazard_tracks d;
    int32_t *d_n = B.get<int32_t>((size_t)t->n_trk);
    int32_t *d_k = n_ev ? B.get<int32_t>(n_ev) : nullptr;
    double *d_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (double *&p : d_ev) if (n_ev) p = B.get<double>(n_ev);
    uint8_t *d_fl = flags ? B.get<uint8_t>(n_fl) : nullptr;
    bool ok = hazard_tracks_upload(B, t, &d) && d_n && (!flags || d_fl);
    if (n_ev) ok = ok && d_k && d_ev[0] && d_ev[1] && d_ev[2] && d_ev[3];
    if (!ok) return fail(ctx, "tcr_landfall_host: device allocation / upload failed");
    if (tcr_landfall_dev(ctx, &d, max_events, d_n, d_k, d_ev[0], d_ev[1], d_ev[2], d_ev[3], d_fl, ctx->stream)) return -1;
    HIPCHK(ctx, hipMemcpyAsync(n_landfall, d_n, sizeof(int32_t) * t->n_trk, hipMemcpyDeviceToHost, ctx->stream));
    if (n_ev) {
        HIPCHK(ctx, hipMemcpyAsync(ev_k, d_k, sizeof(int32_t) * n_ev, hipMemcpyDeviceToHost, ctx->stream));
        double *h_ev[4] = {ev_lon, ev_lat, ev_v, ev_v_inland};
        for (int i = 0; i < 4; ++i) HIPCHK(ctx, hipMemcpyAsync(h_ev[i], d_ev[i], sizeof(double) * n_ev, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (flags) HIPCHK(ctx, hipMemcpyAsync(flags, d_fl, n_fl, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
