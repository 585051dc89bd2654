// Staging: the grids, the static fields and their storage modes, the month slots and the copy pool that feeds them, the masks,
// the fp32 copies, the entropy table — and what the launches read of them (dev_fields, host_eval_k, eval_k_ready).
#pragma once
#include <chrono>

#include "tcr_ctx.h"

using namespace tcr;

namespace {

// An axis is "affine" when x0 + i*dx reproduces every knot bit for bit and every cell's
// reciprocal width 1.0/(x[i+1]-x[i]) is the same double; the kernels then never load knots.
template <typename R>
bool axis_is_affine(const std::vector<R> &x)
{
    const int n = (int)x.size();
    const R x0 = x[0], dx = x[1] - x[0];
    const R rdx = R(1.0) / dx;
    for (int i = 0; i < n; ++i) {
        volatile R prod = (R)i * dx;      // no FMA contraction: mirror the device expression
        volatile R xi = x0 + prod;
        if (xi != x[i]) return false;
    }
    for (int i = 0; i + 1 < n; ++i)
        if (R(1.0) / (x[i + 1] - x[i]) != rdx) return false;
    return true;
}

bool same(const std::vector<double> &a, const double *b, int n)
{
    return (int)a.size() == n && memcmp(a.data(), b, sizeof(double) * n) == 0;
}

// Upload a grid (or check that it equals the one already staged): all month slots
// of one experiment share one wind grid and one thermo grid, as in the reference
// where every Coupled_FAST of a year reads the same env_wnd/thermo datasets.
int stage_grid(tcr_ctx *ctx, GridStore &g, const tcr_grid *in, const char *what)
{
    if (!in || in->nlon < 2 || in->nlat < 2 || !in->lon || !in->lat)
        return fail(ctx, "%s grid: need >= 2 points per axis", what);
    for (int i = 1; i < in->nlon; ++i)
        if (!(in->lon[i] > in->lon[i - 1])) return fail(ctx, "%s grid: lon not strictly increasing", what);
    for (int i = 1; i < in->nlat; ++i)
        if (!(in->lat[i] > in->lat[i - 1])) return fail(ctx, "%s grid: lat not strictly increasing", what);
    if (g.set) {
        if (same(g.lon, in->lon, in->nlon) && same(g.lat, in->lat, in->nlat)) return 0;
        return fail(ctx, "%s grid differs from the grid already staged in this context", what);
    }
    g.lon.assign(in->lon, in->lon + in->nlon);
    g.lat.assign(in->lat, in->lat + in->nlat);
    std::vector<double> rlon(in->nlon - 1), rlat(in->nlat - 1);
    for (int i = 0; i + 1 < in->nlon; ++i) rlon[i] = 1.0 / (in->lon[i + 1] - in->lon[i]);   // fpbspl.f
    for (int i = 0; i + 1 < in->nlat; ++i) rlat[i] = 1.0 / (in->lat[i + 1] - in->lat[i]);
    if (g.d_lon.upload(ctx, g.lon.data(), in->nlon) || g.d_lat.upload(ctx, g.lat.data(), in->nlat) ||
        g.d_rlon.upload(ctx, rlon.data(), in->nlon - 1, 1) || g.d_rlat.upload(ctx, rlat.data(), in->nlat - 1, 1)) return -1;
    g.affine_lon = axis_is_affine(g.lon);
    g.affine_lat = axis_is_affine(g.lat);
    g.set = true;
    return 0;
}

DevAxis dev_axis(const std::vector<double> &x, const double *d_x, const double *d_rx, bool affine)
{
    DevAxis a{};
    a.n = (int)x.size();
    a.affine = affine ? 1 : 0;
    a.x = d_x; a.rx = d_rx;
    a.x0 = x.front(); a.xn = x.back();
    a.dx = x[1] - x[0];
    a.rdx = 1.0 / a.dx;
    a.inv_step = (a.n - 1) / (x.back() - x.front());
    return a;
}

DevGrid dev_grid(const GridStore &g)
{
    DevGrid d{};
    if (!g.set) return d;
    d.nlon = (int)g.lon.size(); d.nlat = (int)g.lat.size();
    d.ax = dev_axis(g.lon, g.d_lon.p, g.d_rlon.p, g.affine_lon);
    d.ay = dev_axis(g.lat, g.d_lat.p, g.d_rlat.p, g.affine_lat);
    return d;
}

int sync_slots(tcr_ctx *ctx)
{
    Staging &S = ctx->sg;
    if (!S.slots_dirty) return 0;
    const size_t n = S.slots.size();
    if (S.d_slots.grow(ctx, n) < 0) return -1;
    std::vector<DevSlot> h(n);
    for (size_t i = 0; i < n; ++i) {
        h[i].wind = S.slots[i].wind.p; h[i].thermo = S.slots[i].thermo.p; h[i].rh = S.slots[i].rh.p;
        h[i].wind32 = S.slots[i].wind32.p; h[i].thermo32 = S.slots[i].thermo32.p;
    }
    if (n) HIPCHK(ctx, copy_sync(ctx->stream, S.d_slots.p, h.data(), sizeof(DevSlot) * n, hipMemcpyHostToDevice));
    S.slots_dirty = false;
    return 0;
}

DevFields dev_fields(const tcr_ctx *ctx)
{
    const Staging &S = ctx->sg;
    DevFields D{};
    D.wg = dev_grid(S.wg); D.tg = dev_grid(S.tg); D.hg = dev_grid(S.hg); D.mg = dev_grid(S.mg);
    D.rg = dev_grid(S.rg);
    D.slots = S.d_slots.p; D.n_slots = (int)S.slots.size();
    D.mask_bits = S.d_mask_bits.p;
    D.all_affine = (S.wg.affine_lon && S.wg.affine_lat && S.tg.affine_lon && S.tg.affine_lat &&
                    S.hg.affine_lon && S.hg.affine_lat &&
                    (!S.split_static || (S.bg.affine_lon && S.bg.affine_lat))) ? 1 : 0;
    return D;
}

int ready(tcr_ctx *ctx, bool need_masks)
{
    if (!ctx) return -1;
    Staging &S = ctx->sg;
    if (!ctx->have_prm) return fail(ctx, "tcr_params_set has not been called");
    if (!S.wg.set || !S.tg.set || S.slots.empty()) return fail(ctx, "no field slot staged (tcr_fields_upload)");
    if (!S.hg.set) return fail(ctx, "static fields not staged (tcr_static_upload)");
    if (need_masks && !S.mg.set) return fail(ctx, "basin masks not staged (tcr_masks_upload)");
    if (S.fields_pending) {
        // the slots staged since the last use: their copies and interleave kernels run on the context's stream, the caller's
        // launches may be on any stream
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        S.fields_pending = false;
    }
    return sync_slots(ctx);
}

// `slot` names a month slot whose fields are staged
bool slot_staged(const tcr_ctx *ctx, int32_t slot)
{
    return slot >= 0 && (size_t)slot < ctx->sg.slots.size() && ctx->sg.slots[slot].wind.p;
}

// kStatPack16 / kStatU8F32 -> the fp64 planes the general (non-affine) kernels read: the same values, widened
__global__ __launch_bounds__(256) void k_static_widen(int mode, const void *__restrict__ nstat, const float *__restrict__ nbathy,
                                                      size_t n_land, size_t n_bathy, double *__restrict__ stat,
                                                      double *__restrict__ land, double *__restrict__ bathy)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (mode == kStatPack16) {
        if (i >= n_land) return;
        const unsigned v = reinterpret_cast<const uint16_t *>(nstat)[i];
        stat[2 * i] = (double)(int)(v & 1u);
        stat[2 * i + 1] = (double)((int)(v >> 1) - kPack16Bias);
    } else if (mode == kStatPack64) {
        if (i >= n_land) return;
        const uint64_t v = reinterpret_cast<const uint64_t *>(nstat)[i];
        stat[2 * i] = (double)(int)((v >> 32) & 0xffu);
        stat[2 * i + 1] = (double)__uint_as_float((unsigned)v);
    } else {
        // (stat != NULL: one shared grid, interleaved; else two planes)
        if (i < n_land) { const double v = (double)reinterpret_cast<const uint8_t *>(nstat)[i]; if (stat) stat[2 * i] = v; else land[i] = v; }
        if (i < n_bathy) { const double v = (double)nbathy[i]; if (stat) stat[2 * i + 1] = v; else bathy[i] = v; }
    }
}

// The planes of one month slot — src = 14 wind planes [nw], 4 thermo planes [nt], rh [nr], in PINNED HOST memory: the
// coalesced plane reads are the transfer — into the slot layouts of tcr_device.h: wind [point][16] (NaN -> 0: _interp_basin_field, bam_track.py:72-74; two pads),
// thermo [point][4], rh as it is.  One thread per grid point.
struct StageSlotArgs {
    const double *src;
    size_t nw, nt, nr;
    double *wind, *thermo, *rh;
};
__global__ __launch_bounds__(256) void k_stage_slot(StageSlotArgs a)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.nw) {
        double v[16];
#pragma unroll
        for (int f = 0; f < 14; ++f) { const double x = a.src[(size_t)f * a.nw + i]; v[f] = (x != x) ? 0.0 : x; }
        v[14] = 0.0; v[15] = 0.0;
        double2 *o = reinterpret_cast<double2 *>(a.wind + i * kWindStride);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = make_double2(v[2 * k], v[2 * k + 1]);
    }
    if (i < a.nt) {
        const double *t = a.src + 14 * a.nw;
        double2 *o = reinterpret_cast<double2 *>(a.thermo + i * kThermoStride);
        o[0] = make_double2(t[i], t[a.nt + i]);
        o[1] = make_double2(t[2 * a.nt + i], t[3 * a.nt + i]);
    }
    if (i < a.nr) a.rh[i] = a.src[14 * a.nw + 4 * a.nt + i];
}

// ---- fp32 staging: float knots (+ reciprocal widths and the affine test in float arithmetic) and float
// copies of the interleaved field layouts, converted on the device from the fp64 arrays already staged
__global__ __launch_bounds__(256) void k_to_f32(const double *__restrict__ src, float *__restrict__ dst, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}

int grid_f32(tcr_ctx *ctx, GridStore &g, const char *what)
{
    if (g.set32) return 0;
    auto one = [&](const std::vector<double> &x, std::vector<float> &x32, DevArray<float> &d_x, DevArray<float> &d_rx, bool *affine) -> int {
        const int n = (int)x.size();
        x32.resize(n);
        for (int i = 0; i < n; ++i) x32[i] = (float)x[i];
        for (int i = 1; i < n; ++i)
            if (!(x32[i] > x32[i - 1])) return fail(ctx, "%s grid: knots are not strictly increasing once rounded to fp32", what);
        std::vector<float> r(n - 1);
        for (int i = 0; i + 1 < n; ++i) r[i] = 1.0f / (x32[i + 1] - x32[i]);
        if (d_x.upload(ctx, x32.data(), (size_t)n) || d_rx.upload(ctx, r.data(), (size_t)n - 1, 1)) return -1;
        *affine = axis_is_affine(x32);
        return 0;
    };
    if (one(g.lon, g.lon32, g.d_lon32, g.d_rlon32, &g.affine_lon32)) return -1;
    if (one(g.lat, g.lat32, g.d_lat32, g.d_rlat32, &g.affine_lat32)) return -1;
    g.set32 = true;
    return 0;
}

int ensure_f32(tcr_ctx *ctx, hipStream_t st)
{
    Staging &S = ctx->sg;
    if (grid_f32(ctx, S.wg, "wind") || grid_f32(ctx, S.tg, "thermo") || grid_f32(ctx, S.hg, "static")) return -1;
    if (S.split_static && grid_f32(ctx, S.bg, "bathymetry")) return -1;
    const size_t nw = S.wg.lon.size() * S.wg.lat.size() * kWindStride;
    const size_t nt = S.tg.lon.size() * S.tg.lat.size() * kThermoStride;
    const size_t nh = S.hg.lon.size() * S.hg.lat.size() * kStaticStride;
    auto conv = [&](const double *src, DevArray<float> &dst, size_t n) -> int {
        if (dst.grow(ctx, n) < 0) return -1;
        hipLaunchKernelGGL(k_to_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst.p, n);
        return 0;
    };
    for (auto &s : S.slots) {
        if (!s.wind.p || !s.f32_stale) continue;
        if (conv(s.wind.p, s.wind32, nw) || conv(s.thermo.p, s.thermo32, nt)) return -1;
        s.f32_stale = false;
        S.slots_dirty = true;
    }
    if (S.stat32_stale && (S.static_mode == kStatF64 || S.static_mode == kStatF64Split)) {
        if (S.split_static) {
            if (conv(S.d_land.p, S.d_land32, nh / kStaticStride)) return -1;
            if (conv(S.d_bathy.p, S.d_bathy32, S.bg.lon.size() * S.bg.lat.size())) return -1;
        } else if (conv(S.d_stat.p, S.d_stat32, nh)) return -1;
        S.stat32_stale = false;
    }
    HIPCHK(ctx, hipGetLastError());
    return sync_slots(ctx);
}

template <typename R> AxisT<R> axis_of(const GridStore &g, bool lon);
template <> AxisT<double> axis_of<double>(const GridStore &g, bool lon)
{
    return lon ? dev_axis(g.lon, g.d_lon.p, g.d_rlon.p, g.affine_lon) : dev_axis(g.lat, g.d_lat.p, g.d_rlat.p, g.affine_lat);
}
template <> AxisT<float> axis_of<float>(const GridStore &g, bool lon)
{
    const std::vector<float> &x = lon ? g.lon32 : g.lat32;
    AxisT<float> a{};
    a.n = (int)x.size();
    a.affine = (lon ? g.affine_lon32 : g.affine_lat32) ? 1 : 0;
    a.x = lon ? g.d_lon32.p : g.d_lat32.p; a.rx = lon ? g.d_rlon32.p : g.d_rlat32.p;
    a.x0 = x.front(); a.xn = x.back();
    a.dx = x[1] - x[0];
    a.rdx = 1.0f / a.dx;
    a.inv_step = (float)(a.n - 1) / (x.back() - x.front());
    return a;
}

// evaluation constants of one precision (copied to LDS by the kernels)
template <typename R>
void host_eval_k(const tcr_ctx *ctx, EvalKT<R> &K, bool *all_affine)
{
    const Staging &S = ctx->sg;
    K.wx = axis_of<R>(S.wg, true); K.wy = axis_of<R>(S.wg, false);
    K.tx = axis_of<R>(S.tg, true); K.ty = axis_of<R>(S.tg, false);
    K.hx = axis_of<R>(S.hg, true); K.hy = axis_of<R>(S.hg, false);
    const bool f64 = std::is_same<R, double>::value;
    if (S.split_static) { K.bx = axis_of<R>(S.bg, true); K.by = axis_of<R>(S.bg, false); }
    else { K.bx = K.hx; K.by = K.hy; }
    switch (S.static_mode) {
    case kStatF64Split:
        K.stat = f64 ? static_cast<const void *>(S.d_land.p) : static_cast<const void *>(S.d_land32.p);
        K.bathy = f64 ? static_cast<const void *>(S.d_bathy.p) : static_cast<const void *>(S.d_bathy32.p);
        break;
    case kStatPack16: case kStatPack64: K.stat = S.d_nstat.p; K.bathy = nullptr; break;
    case kStatU8F32: K.stat = S.d_nstat.p; K.bathy = S.d_nbathy.p; break;
    default:
        K.stat = f64 ? static_cast<const void *>(S.d_stat.p) : static_cast<const void *>(S.d_stat32.p);
        K.bathy = nullptr;
        break;
    }
    eval_k_scalars<R>(ctx->prm, K);
    K.tw_same = (S.wg.lon == S.tg.lon && S.wg.lat == S.tg.lat) ? 1 : 0;       // same knots: the same cells and weights
    K.hb_same = S.split_static ? 0 : 1;
    *all_affine = K.wx.affine && K.wy.affine && K.tx.affine && K.ty.affine && K.hx.affine && K.hy.affine &&
                  K.bx.affine && K.by.affine;
}

// The narrow static modes are instantiated for affine grids only.  A context whose grids are not all affine in the precision
// of the call (a Gaussian latitude axis, say) gets its land / bathymetry widened to the fp64 planes once — the same values —
// and keeps them.
int widen_static(tcr_ctx *ctx, hipStream_t st)
{
    Staging &S = ctx->sg;
    const int mode = S.static_mode;
    if (mode != kStatPack16 && mode != kStatU8F32 && mode != kStatPack64) return 0;
    // (synchronises and frees: never legal inside a stream capture.  tcr_round_dev runs every new descriptor directly before it
    // captures it, and a static re-upload changes the epoch, so the widening always happens in that direct run — guarded anyway)
    if (ctx->capturing) return fail(ctx, "internal: static fields would be widened inside a stream capture");
    const size_t np = S.hg.lon.size() * S.hg.lat.size();
    const size_t nb = S.split_static ? S.bg.lon.size() * S.bg.lat.size() : np;
    if (S.split_static) { if (S.d_land.grow(ctx, np) < 0 || S.d_bathy.grow(ctx, nb) < 0) return -1; }
    else if (S.d_stat.grow(ctx, np * kStaticStride) < 0) return -1;
    hipLaunchKernelGGL(k_static_widen, dim3((unsigned)((std::max(np, nb) + 255) / 256)), dim3(256), 0, st, mode, S.d_nstat.p, S.d_nbathy.p,
                       np, nb, S.d_stat.p, S.d_land.p, S.d_bathy.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    S.d_nstat.reset();
    S.d_nbathy.reset();
    S.static_mode = S.split_static ? kStatF64Split : kStatF64;
    S.static_bytes = sizeof(double) * (np + nb);
    S.stat32_stale = true;
    ++ctx->epoch;
    return 0;
}

template <typename R>
int eval_k_ready(tcr_ctx *ctx, EvalKT<R> &K, bool *affine, hipStream_t st)
{
    host_eval_k<R>(ctx, K, affine);
    const int sm = ctx->sg.static_mode;
    if (!*affine && (sm == kStatPack16 || sm == kStatU8F32 || sm == kStatPack64)) {
        if (widen_static(ctx, st)) return -1;
        if (!std::is_same<R, double>::value && ensure_f32(ctx, st)) return -1;
        host_eval_k<R>(ctx, K, affine);
    }
    return 0;
}

// One month slot: the planes go to the device as they are — copied by the pool into a pinned half, one asynchronous
// transfer — and k_stage_slot interleaves them there (wind NaN -> 0 as _interp_basin_field does, bam_track.py:72-74).
// Nothing here waits for the GPU except for the pinned half it is about to overwrite (two slots back).
// wind / thermo == false: that part is not given (tcr_rh_upload alone / tcr_fields_upload without rh).
int slot_stage(tcr_ctx *ctx, int slot, const tcr_grid *wg, const double *const mean[TCR_NW], const double *const cov[TCR_NCOV],
               const tcr_grid *tg, const double *vpot, const double *chi, const double *mld, const double *strat,
               const tcr_grid *rg, const double *rh_mid)
{
    Staging &S = ctx->sg;
    const bool fields = wg != nullptr, rh = rg != nullptr;
    if (fields && (stage_grid(ctx, S.wg, wg, "wind") || stage_grid(ctx, S.tg, tg, "thermo"))) return -1;
    if (rh && stage_grid(ctx, S.rg, rg, "rh")) return -1;
    if ((size_t)slot >= S.slots.size()) S.slots.resize(slot + 1);
    SlotStore &s = S.slots[slot];
    const size_t nw = fields ? (size_t)wg->nlon * wg->nlat : 0, nt = fields ? (size_t)tg->nlon * tg->nlat : 0;
    const size_t nr = rh ? (size_t)rg->nlon * rg->nlat : 0;
    const size_t need = nw * 14 + nt * 4 + nr;
    if (need > S.h_stage[1].cap) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        S.h_stage[1].reset();             // a failure below leaves "no staging buffer", never a half-built pair at the old capacity
        for (int i = 0; i < 2; ++i) {
            HIPCHK(ctx, S.h_stage[i].alloc(need));
            if (!S.h_stage_ev[i]) HIPCHK(ctx, hipEventCreateWithFlags(&S.h_stage_ev[i], hipEventDisableTiming));
        }
    }
    if (fields && s.wind.grow(ctx, nw * kWindStride) < 0) return -1;
    if (fields && s.thermo.grow(ctx, nt * kThermoStride) < 0) return -1;
    if (rh && s.rh.grow(ctx, nr) < 0) return -1;
    if (!S.pool) S.pool.reset(new CopyPool((ctx->tune.copy_threads > 0 ? std::min(ctx->tune.copy_threads, 16) : 4) - 1));
    const int half = S.h_stage_next;
    S.h_stage_next ^= 1;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    HIPCHK(ctx, hipEventSynchronize(S.h_stage_ev[half]));           // the kernel that last read this half, two uploads ago (long done)
    const double t1 = now();
    double *h = S.h_stage[half].p;
    std::vector<CopyPool::Seg> segs;
    auto add = [&](double *dst, const double *src, size_t n) {
        const size_t chunk = 16384;                                    // 128 KB pieces: a slot is ~75 of them
        for (size_t o = 0; o < n; o += chunk)
            segs.push_back({reinterpret_cast<char *>(dst + o), reinterpret_cast<const char *>(src + o), sizeof(double) * std::min(chunk, n - o)});
    };
    if (fields) {
        for (int f = 0; f < 14; ++f) add(h + (size_t)f * nw, f < 4 ? mean[f] : cov[f - 4], nw);
        const double *th[4] = {vpot, chi, mld, strat};
        for (int k = 0; k < 4; ++k) add(h + 14 * nw + (size_t)k * nt, th[k], nt);
    }
    if (rh) add(h + 14 * nw + 4 * nt, rh_mid, nr);
    S.pool->run(segs);
    const double t2 = now();
    // The interleave kernel reads the pinned half ITSELF, over the link (hipHostMalloc memory is mapped into the device's
    // address space): no copy engine, no landing buffer, one stream.  A transfer followed by the kernel that consumes it makes
    // the next transfer wait for that kernel — a copy-engine job depending on a compute-queue signal, which the runtime
    // resolves on a host thread: inside run_downscaling that hop took 1-2 ms per slot (tools/stage_in_run_probe.py) although
    // the 9.9 MB transfer itself takes 0.26 ms.
    const double t3 = now();
    StageSlotArgs a{};
    a.src = h; a.nw = nw; a.nt = nt; a.nr = nr; a.wind = s.wind.p; a.thermo = s.thermo.p; a.rh = s.rh.p;
    const size_t nmax = std::max(nw, std::max(nt, nr));
    hipLaunchKernelGGL(k_stage_slot, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(S.h_stage_ev[half], ctx->stream));
    const double t4 = now();
    S.stage_ms[0] += t1 - t0; S.stage_ms[1] += t2 - t1; S.stage_ms[2] += t3 - t2; S.stage_ms[3] += t4 - t3; S.stage_ms[4] += 1.0;
    if (fields) s.f32_stale = true;
    S.slots_dirty = true;
    S.fields_pending = true;
    return 0;
}

}  // namespace

extern "C" {

int tcr_static_store(tcr_ctx *ctx, int32_t pref)
{
    if (!ctx) return -1;
    if (pref != 0 && pref != 1) return fail(ctx, "tcr_static_store: 0 (auto) or 1 (fp64 planes)");
    ctx->sg.static_pref = pref;
    return 0;
}

int tcr_static_info(tcr_ctx *ctx, int32_t *mode, int64_t *bytes)
{
    if (!ctx) return -1;
    if (!ctx->sg.hg.set) return fail(ctx, "static fields not staged (tcr_static_upload)");
    if (mode) *mode = ctx->sg.static_mode;
    if (bytes) *bytes = (int64_t)ctx->sg.static_bytes;
    return 0;
}

int tcr_static_upload2(tcr_ctx *ctx, const tcr_grid *lg, const double *land, const tcr_grid *bg, const double *bathy)
{
    if (!enter(ctx)) return -1;
    Staging &S = ctx->sg;
    if (!land || !bathy || !lg || !bg) return fail(ctx, "tcr_static_upload: NULL argument");
    const bool shared = lg->nlon == bg->nlon && lg->nlat == bg->nlat && lg->lon && bg->lon && lg->lat && bg->lat &&
                        memcmp(lg->lon, bg->lon, sizeof(double) * lg->nlon) == 0 &&
                        memcmp(lg->lat, bg->lat, sizeof(double) * lg->nlat) == 0;
    if (S.hg.set && shared == S.split_static)
        return fail(ctx, "static fields were staged %s before; a context keeps one arrangement", S.split_static ? "on two grids" : "on one grid");
    if (stage_grid(ctx, S.hg, lg, shared ? "static" : "land")) return -1;
    if (!shared && stage_grid(ctx, S.bg, bg, "bathymetry")) return -1;
    const size_t np = (size_t)lg->nlon * lg->nlat, nb = (size_t)bg->nlon * bg->nlat;
    // Exact narrow storage where the VALUES allow it (the reference's land.nc is int8 0 / 1 on a 0.125-degree grid,
    // intensity/geo.py:23-34; bathymetry products are whole metres or float32): the kernels widen to the same doubles, so
    // nothing downstream — the `land == 1` decision included — can tell the difference.
    bool land01 = true, land_u8 = true, bathy_i15 = true, bathy_f32 = true;
    for (size_t i = 0; i < np && land_u8; ++i) {
        const double v = land[i];
        if (!(v >= 0.0 && v <= 255.0 && v == (double)(int)v)) land_u8 = false;
        if (v != 0.0 && v != 1.0) land01 = false;
    }
    for (size_t i = 0; i < nb && bathy_f32; ++i) {
        const double v = bathy[i];
        if (!((double)(float)v == v)) bathy_f32 = false;                  // (a NaN keeps the fp64 planes)
        if (!(v >= -(double)kPack16Bias && v < (double)kPack16Bias && v == (double)(int)v)) bathy_i15 = false;
    }
    int mode = shared ? kStatF64 : kStatF64Split;
    if (S.static_pref == 0) {
        if (shared && land_u8 && land01 && bathy_f32 && bathy_i15) mode = kStatPack16;
        else if (shared && land_u8 && bathy_f32) mode = kStatPack64;
        else if (land_u8 && bathy_f32) mode = kStatU8F32;
    }
    // a context may be re-staged with other planes (another mode, even): start from nothing (freed behind a synchronisation;
    // a captured round holds the old planes' addresses)
    auto drop = [&](auto &plane) -> int {
        if (plane.p) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); plane.reset(); ++ctx->epoch; }
        return 0;
    };
    if (drop(S.d_stat) || drop(S.d_land) || drop(S.d_bathy) || drop(S.d_stat32) || drop(S.d_land32) || drop(S.d_bathy32) ||
        drop(S.d_nstat) || drop(S.d_nbathy)) return -1;
    if (mode == kStatPack16) {
        std::vector<uint16_t> h(np + 8, 0);
        for (size_t i = 0; i < np; ++i) h[i] = (uint16_t)((((int)bathy[i] + kPack16Bias) << 1) | (int)land[i]);
        if (S.d_nstat.upload(ctx, reinterpret_cast<const uint8_t *>(h.data()), sizeof(uint16_t) * h.size())) return -1;
        S.static_bytes = sizeof(uint16_t) * np;
    } else if (mode == kStatPack64) {
        std::vector<uint64_t> h(np + 2, 0);
        for (size_t i = 0; i < np; ++i) {
            const float b = (float)bathy[i];
            uint32_t bits;
            memcpy(&bits, &b, 4);
            h[i] = (uint64_t)bits | ((uint64_t)(uint8_t)(int)land[i] << 32);
        }
        if (S.d_nstat.upload(ctx, reinterpret_cast<const uint8_t *>(h.data()), sizeof(uint64_t) * h.size())) return -1;
        S.static_bytes = sizeof(uint64_t) * np;
    } else if (mode == kStatU8F32) {
        std::vector<uint8_t> hl(np + 8, 0);
        std::vector<float> hb(nb + 4, 0.f);
        for (size_t i = 0; i < np; ++i) hl[i] = (uint8_t)(int)land[i];
        for (size_t i = 0; i < nb; ++i) hb[i] = (float)bathy[i];
        if (S.d_nstat.upload(ctx, hl.data(), hl.size()) || S.d_nbathy.upload(ctx, hb.data(), hb.size())) return -1;
        S.static_bytes = np + sizeof(float) * nb;
    } else if (shared) {
        std::vector<double> h(np * kStaticStride);
        for (size_t i = 0; i < np; ++i) { h[i * 2] = land[i]; h[i * 2 + 1] = bathy[i]; }
        if (S.d_stat.upload(ctx, h.data(), h.size())) return -1;
        S.static_bytes = sizeof(double) * h.size();
    } else {
        if (S.d_land.upload(ctx, land, np) || S.d_bathy.upload(ctx, bathy, nb)) return -1;
        S.static_bytes = sizeof(double) * (np + nb);
    }
    S.split_static = !shared;
    S.static_mode = mode;
    S.stat32_stale = true;
    return 0;
}

int tcr_static_upload(tcr_ctx *ctx, const tcr_grid *hg, const double *land, const double *bathy)
{
    return tcr_static_upload2(ctx, hg, land, hg, bathy);
}

int tcr_slot_upload(tcr_ctx *ctx, int slot, const tcr_grid *wg, const double *const mean[TCR_NW],
                    const double *const cov[TCR_NCOV], const tcr_grid *tg, const double *vpot,
                    const double *chi, const double *mld, const double *strat, const tcr_grid *rg, const double *rh_mid)
{
    if (!enter(ctx)) return -1;
    if (slot < 0 || slot >= 4096) return fail(ctx, "tcr_slot_upload: slot out of range");
    if (!wg || !tg || !mean || !cov || !vpot || !chi || !mld || !strat) return fail(ctx, "tcr_slot_upload: NULL plane");
    for (int f = 0; f < 14; ++f)
        if (!(f < 4 ? mean[f] : cov[f - 4])) return fail(ctx, "tcr_slot_upload: NULL wind plane");
    if ((rg == nullptr) != (rh_mid == nullptr)) return fail(ctx, "tcr_slot_upload: rh grid and plane go together");
    return slot_stage(ctx, slot, wg, mean, cov, tg, vpot, chi, mld, strat, rg, rh_mid);
}

int tcr_fields_upload(tcr_ctx *ctx, int slot, const tcr_grid *wg, const double *const mean[TCR_NW],
                      const double *const cov[TCR_NCOV], const tcr_grid *tg, const double *vpot,
                      const double *chi, const double *mld, const double *strat)
{
    return tcr_slot_upload(ctx, slot, wg, mean, cov, tg, vpot, chi, mld, strat, nullptr, nullptr);
}

int tcr_rh_upload(tcr_ctx *ctx, int slot, const tcr_grid *rg, const double *rh_mid)
{
    if (!enter(ctx)) return -1;
    if (slot < 0 || slot >= 4096) return fail(ctx, "tcr_rh_upload: slot out of range");
    if (!rg || !rh_mid) return fail(ctx, "tcr_rh_upload: NULL plane");
    return slot_stage(ctx, slot, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rg, rh_mid);
}

int tcr_stage_timing(tcr_ctx *ctx, double ms[5], int32_t reset)
{
    if (!ctx || !ms) return -1;
    for (int i = 0; i < 5; ++i) { ms[i] = ctx->sg.stage_ms[i]; if (reset) ctx->sg.stage_ms[i] = 0.0; }
    return 0;
}

int tcr_masks_upload(tcr_ctx *ctx, const tcr_grid *mg, const uint8_t *run_mask,
                     const uint8_t *const basin_masks[TCR_N_BASINS])
{
    if (!enter(ctx)) return -1;
    if (!run_mask || !basin_masks) return fail(ctx, "tcr_masks_upload: NULL mask");
    if (stage_grid(ctx, ctx->sg.mg, mg, "mask")) return -1;
    const size_t np = (size_t)mg->nlon * mg->nlat;
    static_assert(TCR_N_BASINS == 7, "seven basin masks + the run basin's fill one byte");
    std::vector<uint8_t> bits(np, 0);
    for (int b = 0; b < TCR_N_BASINS; ++b) {
        if (!basin_masks[b]) return fail(ctx, "tcr_masks_upload: NULL basin mask");
        for (size_t i = 0; i < np; ++i) bits[i] |= (uint8_t)((basin_masks[b][i] ? 1u : 0u) << b);
    }
    for (size_t i = 0; i < np; ++i) bits[i] |= (uint8_t)((run_mask[i] ? 1u : 0u) << 7);
    return ctx->sg.d_mask_bits.upload(ctx, bits.data(), np);
}

int tcr_entropy_table_upload(tcr_ctx *ctx, int32_t np, int32_t ns, const double *p, const double *s, const double *T)
{
    if (!ctx) return -1;
    if (np < 2 || ns < 2 || !p || !s || !T) return fail(ctx, "tcr_entropy_table_upload: bad argument");
    for (int i = 1; i < np; ++i) if (!(p[i] > p[i - 1])) return fail(ctx, "tcr_entropy_table_upload: pressure axis must ascend");
    for (int i = 1; i < ns; ++i) if (!(s[i] > s[i - 1])) return fail(ctx, "tcr_entropy_table_upload: entropy axis must ascend");
    if (!enter(ctx)) return -1;
    DevArray<double> &tab = ctx->sg.d_tab;
    tab.reset();
    if (tab.grow(ctx, (size_t)np + ns + (size_t)np * ns) < 0) return -1;
    HIPCHK(ctx, copy_sync(ctx->stream, tab.p, p, sizeof(double) * np, hipMemcpyHostToDevice));
    HIPCHK(ctx, copy_sync(ctx->stream, tab.p + np, s, sizeof(double) * ns, hipMemcpyHostToDevice));
    HIPCHK(ctx, copy_sync(ctx->stream, tab.p + np + ns, T, sizeof(double) * (size_t)np * ns, hipMemcpyHostToDevice));
    ctx->sg.tab_np = np; ctx->sg.tab_ns = ns;
    return 0;
}

}  // extern "C"
