// C-ABI host side of libtcrisk_hip.so (see include/tcrisk_hip.h for the contract and the reference interface each entry
// point replaces): the one translation unit of the library.  This file is the list of its parts in dependency order, the
// life of a context (create, destroy, parameters) and the launch-shape knobs; every other subject has a file of its own.
#include <hip/hip_runtime.h>

#include <cstdlib>

// kernels
#include "tcr_kernels.hip"
#include "tcr_seed.hip"
#include "tcr_compact.hip"
#include "tcr_prep.hip"
#include "tcr_thermo.hip"
#ifdef TCR_EXPERIMENTS
#include "tcr_experiments.h"       // scheduling probes and per-call environment knobs: tools/build_variant.py NAME -DTCR_EXPERIMENTS
#endif

// host layer ("Map of the host layer")
#include "tcr_host.h"                    // fail, HIPCHK, copy_sync, the owners of device and pinned memory, DevBuf, the variant dispatch, enter
#include "tcr_ctx.h"                     // the context: staging, integrator workspaces, round and graphs, timing and trace, analyses
#include "tcr_stage.hip"                 // grids, static fields and their storage modes, month slots, masks, fp32 copies, entropy table
#include "tcr_integrate.hip"             // launch shapes, forcing table, integrate_impl, tcr_integrate_*, timing, probes
#include "tcr_preprocess.hip"            // potential intensity, chi / rh, wind statistics
#include "tcr_round.hip"                 // seed, compact, cell order, gather, stats, pack, seed histogram; tcr_round_dev and its graphs

namespace {

// The launch-shape knobs a context starts from: the environment, read ONCE (tcr_ctx_create); tcr_tune_set replaces them.
long env_long(const char *name, long dflt)
{
    const char *e = getenv(name);
    return e ? atol(e) : dflt;
}
tcr_tune tune_from_env()
{
    tcr_tune t;
    t.waves = (int32_t)env_long("TCR_WAVES", -1);
    t.park = (int32_t)std::min<long>(env_long("TCR_PARK", -1), 63);     // (tcr_tune_set's own bound: a get / modify / set round trip must not fail on it)
    t.park_final = (int32_t)env_long("TCR_PARK_FINAL", -1);
    t.table_segments = (int32_t)env_long("TCR_TABLE_SEGMENTS", -1);
    t.prune = (int32_t)env_long("TCR_PRUNE", -1);
    t.emit_grid_cap = (int32_t)env_long("TCR_EMIT_GRID_CAP", -1);
    t.copy_threads = (int32_t)env_long("TCR_COPY_THREADS", -1);
    t.table_factors = (int32_t)env_long("TCR_TABLE_FACTORS", -1);
    return t;
}

}  // namespace

extern "C" {

int tcr_abi_version(void) { return TCR_ABI_VERSION; }

const char *tcr_last_error(const tcr_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int tcr_ctx_create(int device, tcr_ctx **out)
{
    if (!out) return fail(nullptr, "tcr_ctx_create: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, "no HIP device available (%s); this library has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= count) return fail(nullptr, "tcr_ctx_create: device index out of range");
    tcr_ctx *ctx = new tcr_ctx();
    ctx->device = device;
    ctx->tune = tune_from_env();
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&ctx->stream) != hipSuccess) {
        delete ctx;
        return fail(nullptr, "tcr_ctx_create: hipSetDevice/hipStreamCreate failed");
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) {
        ctx->cu_count = prop.multiProcessorCount;
        if (prop.sharedMemPerBlock < kCellScanLds) {
            delete ctx;
            return fail(nullptr, "tcr_ctx_create: this library is built for gfx950 (160 KB of LDS per CU); the device offers less than k_cell_scan's 67 KB per workgroup");
        }
    }
    if (ctx->ws.d_queue.alloc_bytes(kQueueWords * sizeof(unsigned long long)) != hipSuccess ||
        ctx->ws.d_tc_count.alloc_bytes(64) != hipSuccess || ctx->rd.d_round_key.alloc_bytes(64) != hipSuccess) {
        delete ctx;
        return fail(nullptr, "tcr_ctx_create: hipMalloc failed");
    }
    *out = ctx;
    return 0;
}

// (every member of the context frees what it owns; the stream goes last, with the context's base)
int tcr_ctx_destroy(tcr_ctx *ctx)
{
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
    return 0;
}

int tcr_params_set(tcr_ctx *ctx, const tcr_params *p)
{
    if (!ctx || !p) return -1;
    if (p->n_series < 1 || p->n_series > TCR_MAX_SERIES) return fail(ctx, "n_series out of range");
    if (p->n_steps < 2 || p->n_steps > 4096) return fail(ctx, "n_steps must be in [2, 4096]");
    if (p->max_rk_steps < 0 || p->max_rk_steps > 4096) return fail(ctx, "max_rk_steps out of range");
    if (!(p->total_time > 0) || !(p->dt_out > 0)) return fail(ctx, "total_time and dt_out must be positive");
    ctx->prm = *p;
    ctx->have_prm = true;
    ++ctx->epoch;
    // Periodic Fourier kernel when the series period is a whole number of output intervals
    // and the output times are exactly k*dt_out (np.linspace with an exact step).
    if (!enter(ctx)) return -1;
    ctx->ws.fs_period = 0;
    const double per = p->T_Fs / p->dt_out;
    const int iper = (int)per;
    const bool regular = p->dt_out * (double)(p->n_steps - 1) == p->total_time;
    if (regular && iper >= 2 && iper <= 4096 && (double)iper == per && (double)iper * p->dt_out == p->T_Fs) {
        std::vector<double2> tab(iper);
        const long double two_pi = 6.283185307179586476925286766559005768L;
        for (int j = 0; j < iper; ++j) {
            const long double ang = two_pi * (long double)j / (long double)iper;
            tab[j] = make_double2((double)sinl(ang), (double)cosl(ang));
        }
        ctx->ws.d_sc_table.reset();
        if (ctx->ws.d_sc_table.upload(ctx, tab.data(), (size_t)iper)) return -1;
        ctx->ws.fs_period = iper;
    }
    return 0;
}

int tcr_schedule_set(tcr_ctx *ctx, int32_t storms_per_lane)
{
    if (!ctx) return -1;
    if (storms_per_lane < 1 || storms_per_lane > 64) return fail(ctx, "tcr_schedule_set: storms_per_lane must be in [1, 64]");
    if (storms_per_lane != ctx->storms_per_lane) ++ctx->epoch;        // captured rounds hold the launch shape
    ctx->storms_per_lane = storms_per_lane;
    return 0;
}

int tcr_tune_set(tcr_ctx *ctx, const tcr_tune *t)
{
    if (!ctx || !t) return -1;
    if (t->park > 63) return fail(ctx, "tcr_tune_set: park must be < 64");
    if (t->copy_threads != ctx->tune.copy_threads) ctx->sg.pool.reset();       // (the next slot upload starts the pool it asks for)
    ctx->tune = *t;
    ++ctx->epoch;                  // captured rounds hold the launch shape
    return 0;
}

int tcr_tune_get(tcr_ctx *ctx, tcr_tune *t)
{
    if (!ctx || !t) return -1;
    *t = ctx->tune;
    return 0;
}

}  // extern "C"

#include "tcr_comm.hip"                  // multi-GPU exchange (RCCL, loaded at run time)
#include "tcr_sitescan.h"                // what the per-site analyses share: tile scan, culling caps, chunk table, workspaces
#include "tcr_hazard.hip"                // site wind hazard (near-site intensity, exceedance counts)
#include "tcr_landfall.hip"              // landfall detection (sea -> land steps of the model's land decision)
#include "tcr_climatology.hip"           // track climatology (track, exceedance, genesis, LMI density and PDI per cell)
#include "tcr_windfield.hip"             // wind footprint (peak wind at sites from a radial profile, exceedance counts)
#include "tcr_loss.hip"                  // portfolio loss (damage function on the footprint, summed over sites inside the scan)
#include "tcr_rainfall.hip"              // rainfall footprint (R-CLIPER rain rate integrated along the track, or its peak, at sites)
#include "tcr_compound.hip"              // compound wind-rain hazard (both footprints in one scan, joint exceedance counts)
#include "tcr_duration.hip"              // wind duration (hours at or above wind levels at sites: integer half-weights per level)
#include "tcr_directional.hip"           // directional wind (peak footprint wind from each compass sector at sites: a max per sector)
#include "tcr_accumulation.hip"          // rain accumulation windows (peak rain depth in any m consecutive samples at sites: a ring of running depths per lane)
#include "tcr_approach.hip"              // closest approach (the nearest record of every storm to every site and what the storm was doing there: an argmin with a payload)
#include "tcr_select.hip"                // row selection (the k-th largest of every row of a per-storm plane: return levels)
#include "tcr_tail.hip"                  // row tail fit (a GPD fitted to the k largest of every row: return levels past the record)
#include "tcr_rowpack.hip"               // row packing (the entries of every row of a per-storm plane at or above a floor, as CSR: event footprints)
#include "tcr_joint.hip"                 // joint hazard (one bit per (site, level, unit) of a per-storm plane, popcounts of ANDed bit rows: co-exceedance between sites)
