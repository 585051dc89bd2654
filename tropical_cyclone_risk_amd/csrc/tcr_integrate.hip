// The integrator behind tcr_integrate_*: launch shapes, the forcing table, the chain of k_integrate passes and the
// post-processing (integrate_impl); its timing and pass statistics; the probes (rhs, init_m, math, fourier_table).
#pragma once
#include <cmath>

#include "tcr_stage.hip"

namespace {

// Number of persistent waves of k_integrate.  Lanes pull storms from a queue, so fewer
// lanes than storms is fine (and balances storm lifetimes); up to one wave per SIMD while
// the batch is small, two per SIMD once every lane would still get several storms.
unsigned integrate_waves(const tcr_ctx *ctx, int64_t n, int wps)
{
    // one wave per SIMD per launch also when the register budget allows wps > 1 resident waves (fp32): the second
    // slot is for the waves of the batches other streams have in flight, and a launch of more waves than storms / 64
    // would leave lanes without work from the start
    (void)wps;
    const int64_t simds = (int64_t)ctx->cu_count * 4;
    int64_t waves = (n + kWave - 1) / kWave;
    if (ctx->tune.waves > 0) return (unsigned)(ctx->tune.waves < waves ? ctx->tune.waves : waves);
    if (waves > simds) waves = (n >= simds * kWave * 4) ? 2 * simds : simds;
    else if (ctx->storms_per_lane > 1) {
        // a batch that does not fill the chip, on a context set up for throughput (tcr_schedule_set): fewer waves whose lanes
        // take several storms in turn — the queue balances the lifetimes, so a batch costs a third of the SIMD time (lane
        // utilisation 0.44 -> 0.8) and leaves SIMDs to the batches other streams have in flight, for a ~1.4x longer chain
        const int64_t w = (n + (int64_t)kWave * ctx->storms_per_lane - 1) / ((int64_t)kWave * ctx->storms_per_lane);
        waves = std::max<int64_t>(std::min<int64_t>(waves, 16), w);
    }
    return (unsigned)(waves < 1 ? 1 : waves);
}

// Tail compaction of k_integrate: a wave parks its storms once fewer than this many lanes are
// live and the queue is empty.  Only worth it when the launch fills the chip (one wave per SIMD):
// it trades latency of the chain (pass barriers) for SIMD time, and SIMD time is only scarce then.
// tcr_tune.park = 0 disables the chain (one launch runs every storm to its end), k > 0 forces k.
int park_threshold(const tcr_ctx *ctx, unsigned waves, int wps)
{
    if (ctx->tune.park >= 0) return ctx->tune.park > 63 ? 63 : ctx->tune.park;
    (void)wps;
    // 12: measured on 100 000-storm steps (4 streams, segmented forcing table) — threshold 8 / 12 / 16 / 24 give 1.41 / 1.39 / 1.39 /
    // 1.38 ms per step and chains of 2.20 / 2.14-2.20 / 2.20-2.24 / 2.31-2.34 ms (5 / 5 / 6 / 7 passes): a higher threshold buys lane
    // utilisation (0.69 ... 0.83) with pass barriers; 12 has the shortest chain at (within noise) the best step time
    return waves >= (unsigned)ctx->cu_count * 4u ? 12 : 0;
}

// TCR_PASS_FILL=p (experiment builds): passes after the first launch only p % as many lanes as they have parked storms
// (k_integrate, fill_pct)
int pass_fill_pct()
{
#ifdef TCR_EXPERIMENTS
    return tcr_exp::pass_fill_pct();
#else
    return 100;
#endif
}
// np.linspace(0, total_time, n_steps)[i] as the kernels form it (ts_at)
double ts_host(const tcr_params &P, int i)
{
    return (i == P.n_steps - 1) ? P.total_time : (double)i * (P.total_time / (double)(P.n_steps - 1));
}

constexpr size_t kQueueWords = 6 * kMaxPasses;     // heads, parked counts, 4 occupancy counters per pass
// A pass this small runs to the end.  Default: one wave per CU (256 on MI355X) — for a chip-filling batch that is three passes
// (1 024, 1 024 behind the table's second segment, 176 waves) instead of the five of rounds 2-5 (… 30, 5 waves; the default was
// 8): the two tiny passes held 0.2 % of the SIMD time and each cost a dispatch in the chain.  Round 6, same box: exclusive
// chain -4 %, one-stream step -5 %, 12-stream step -1…1.5 %, SIMD time +1 % (profiles/r06_dispatch_and_knobs.txt).
unsigned park_final_waves(const tcr_ctx *ctx)
{
    return ctx->tune.park_final > 0 ? (unsigned)ctx->tune.park_final : (unsigned)std::max(8, ctx->cu_count);
}

// stage trace: an event labelled with the stage that has just been enqueued (not while a round is being captured)
int stage_mark(tcr_ctx *ctx, hipStream_t st, int id)
{
    Trace &T = ctx->tr;
    if (!T.stage_trace || ctx->capturing) return 0;
    if (T.st_used == T.st_pool.size()) {
        const size_t old = T.st_pool.size();
        T.st_pool.resize(old + 256, nullptr);
        T.st_id.resize(old + 256, 0);
        for (size_t i = old; i < T.st_pool.size(); ++i) HIPCHK(ctx, hipEventCreate(&T.st_pool[i]));
    }
    T.st_id[T.st_used] = id;
    HIPCHK(ctx, hipEventRecord(T.st_pool[T.st_used], st));
    ++T.st_used;
    return 0;
}
#define STAGE(id) do { if (stage_mark(ctx, (hipStream_t)st, id)) return -1; } while (0)

// per timed call: [0] start, [1] table (first segment) written, [2] integration chain done, [3] post-processing done,
// [4], [5] around the table's second segment inside the chain (recorded back to back when there is none)
constexpr size_t kEvPerCall = 6;
int timing_events(tcr_ctx *ctx, hipEvent_t **quad)
{
    Trace &T = ctx->tr;
    if (T.ev_used + kEvPerCall > T.ev_pool.size()) {
        const size_t old = T.ev_pool.size();
        T.ev_pool.resize(old + 64, nullptr);
        for (size_t i = old; i < T.ev_pool.size(); ++i) HIPCHK(ctx, hipEventCreate(&T.ev_pool[i]));
    }
    *quad = &T.ev_pool[T.ev_used];
    T.ev_used += kEvPerCall;
    return 0;
}

// ms[0] forcing table (both segments), ms[1] integration chain without the table's second segment, ms[2] post-processing
int timing_of_call(tcr_ctx *ctx, hipEvent_t *q, double ms[3])
{
    float f[3] = {0.f, 0.f, 0.f}, seg = 0.f;
    for (int i = 0; i < 3; ++i) HIPCHK(ctx, hipEventElapsedTime(&f[i], q[i], q[i + 1]));
    HIPCHK(ctx, hipEventElapsedTime(&seg, q[4], q[5]));
    ms[0] = f[0] + seg; ms[1] = f[1] - seg; ms[2] = f[2];
    return 0;
}

template <typename R>
void launch_integrate(const KArgsT<R> &a, bool affine, bool probe, int sm, unsigned waves, hipStream_t st)
{
    with_eval_variant(affine, sm, [&](auto A, auto S) {
        constexpr bool AF = decltype(A)::value;
        constexpr int SM = decltype(S)::value;
        if constexpr (std::is_same<R, double>::value) {                // the decision probe is an fp64 instrument
            if (probe) { hipLaunchKernelGGL((k_integrate<R, AF, true, SM>), dim3(waves), dim3(kWave), 0, st, a); return; }
        }
        hipLaunchKernelGGL((k_integrate<R, AF, false, SM>), dim3(waves), dim3(kWave), 0, st, a);
    });
}

// Outputs of one precision: tcr_tracks (double planes) or tcr_tracks_f32 (float planes), same layout
template <typename R>
struct TracksT {
    R *lon, *lat, *v, *m, *vmax, *envw;
    int32_t *n_valid, *status, *flags, *nfev, *n_accept, *n_reject, *pad_state;
    int32_t tc_rows_only;
};
template <typename R, typename T>
TracksT<R> tracks_of(const T *o)
{
    TracksT<R> t{};
    t.lon = o->lon; t.lat = o->lat; t.v = o->v; t.m = o->m; t.vmax = o->vmax; t.envw = o->envw;
    t.n_valid = o->n_valid; t.status = o->status; t.flags = o->flags; t.nfev = o->nfev;
    t.n_accept = o->n_accept; t.n_reject = o->n_reject; t.pad_state = o->pad_state; t.tc_rows_only = o->tc_rows_only;
    return t;
}

// The forcing table can be written in two segments of 12 column tiles (192 samples) each: the first for every storm before
// the chain starts, the second only for the storms the first integration pass parks.
constexpr int kFsSegSamples = kFsMfmaWaves * kFsMfmaColTiles * 16;
enum FsPart { kFsAll = -1, kFsFirst = 0, kFsRest = 1 };
bool fourier_on_matrix_cores(const tcr_ctx *ctx)
{
    const tcr_params &P = ctx->prm;
    return TCR_FS_MFMA && ctx->ws.fs_period > 0 && 2 * P.n_series <= 4 * kFsMfmaKSteps && P.n_steps <= kFsMfmaMaxSamples;
}

// part = kFsRest: rows are the storms of the park list `park` (count on the device, at most n)
template <typename R>
int launch_fourier(tcr_ctx *ctx, int64_t n, const int64_t *n_dev, const double *phases, R *fs, hipStream_t st,
                   FsPart part = kFsAll, const double *park = nullptr, const unsigned long long *park_count = nullptr,
                   const BatchReset *reset = nullptr)
{
    IntegrateWs &W = ctx->ws;
    // the batch's counters are zeroed by the batch's first kernel that runs anyway — the fused table kernel, or the phase-factor
    // kernel when tcr_tune.table_factors = 0 — else by a launch of their own
    BatchReset z{};
    if (reset) z = *reset;
    if (reset && !(W.fs_period > 0 && fourier_on_matrix_cores(ctx)))
        hipLaunchKernelGGL(k_batch_reset, dim3((unsigned)((std::max<int64_t>(z.n_flags, z.queue_words) + 255) / 256)), dim3(256), 0, st, z);
    const tcr_params &P = ctx->prm;
    if (W.fs_period > 0) {
        const size_t lds = sizeof(double2) * (size_t)W.fs_period;
        const int64_t nf = n * 4 * (int64_t)P.n_series;
        // table_factors: the table kernel forms its A fragments from the phases itself; d_pf exists only for the paths that read it
        const bool fused = fourier_on_matrix_cores(ctx) && ctx->tune.table_factors != 0;
        if (!fused && part != kFsRest) {        // (kFsRest reads what the first segment's call left in d_pf: no reallocation in between)
            if (W.d_pf.grow(ctx, (size_t)nf) < 0) return -1;
        } else if (!fused && !W.d_pf.p) return fail(ctx, "internal: second table segment without the first");
        if (fourier_on_matrix_cores(ctx)) {
            // matrix-core form: phase factors in MFMA fragment order (4 KB per 4 storms <= the 3.84 KB of d_pf's layout + padding)
            const int64_t tiles = (n + 3) / 4;
            // kFsRest: the second segment for the parked storms is ONE launch (round 6; three until then): the table kernel reads the
            // storm ids straight out of the park records (word 13 of each, k_integrate's park()) and forms every storm's phase
            // factors from its phases — or, table_factors = 0, picks them out of the fragments the first segment's
            // k_phase_factors_frag wrote for the whole batch: d_pf is not written between the two segments (only this function
            // writes it, and a batch's two calls are on one stream)
            const int64_t *list = nullptr;
            int list_stride = 1;
            if (part == kFsRest) {
                list = reinterpret_cast<const int64_t *>(park) + 13;
                list_stride = kParkRec;
            } else if (!fused) {
                if (W.d_pf.grow(ctx, (size_t)tiles * kFsMfmaKSteps * 32) < 0) return -1;
                hipLaunchKernelGGL(k_phase_factors_frag, dim3((unsigned)std::min<int64_t>(tiles, 8192)), dim3(256), 0, st, P, n, n_dev, phases,
                                   reinterpret_cast<double *>(W.d_pf.p), nullptr, nullptr, z);
            }
            const double *p = fused ? phases : reinterpret_cast<const double *>(W.d_pf.p);
            const int groups = part == kFsAll ? kFsMfmaColGroups : 1;
            // workgroups per launch: TCR_FS_WGS=<total> overrides (scheduling experiment: a workgroup's two 191-register waves
            // keep integrator waves of other batches off their SIMDs)
            int64_t want = (int64_t)ctx->cu_count * kFsMfmaWgsPerCu * (4 / kFsMfmaWaves) / groups;
#ifdef TCR_EXPERIMENTS
            want = tcr_exp::fs_workgroups(want, groups);
#endif
            const unsigned wgs = (unsigned)std::min<int64_t>(tiles, std::max<int64_t>(1, want));
            const dim3 grid(wgs, groups), block(64 * kFsMfmaWaves);
            const BatchReset none{};
            with_flags(part == kFsRest, fused, [&](auto REST, auto FUSED) {
                constexpr bool rest = decltype(REST)::value, fu = decltype(FUSED)::value;
                hipLaunchKernelGGL((k_fourier_mfma<R, rest, fu>), grid, block, 0, st, P, n, n_dev, W.fs_period, W.d_sc_table.p, p, fs,
                                   rest ? 1 : 0, list, list_stride, park_count, (fu && !rest) ? z : none);
            });
        } else {
            hipLaunchKernelGGL(k_phase_factors, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, P, n, n_dev, phases, W.d_pf.p);
            hipLaunchKernelGGL(k_fourier_periodic<R>, dim3((unsigned)n), dim3(kFsThreads), lds, st, P, n, n_dev,
                               W.fs_period, W.d_sc_table.p, W.d_pf.p, fs);
        }
    } else {
        const int64_t total = n * (int64_t)P.n_steps;
        hipLaunchKernelGGL(k_fourier_direct<R>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P, n, n_dev, phases, fs);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// The per-candidate body of run_tracks for a batch (see tcr_integrate_dev in the header), in precision R.
// stats: optional device counter block (TCR_N_STATS words) the batch's sums are added to by k_flags (tcr_round_dev)
template <typename R>
int integrate_impl(tcr_ctx *ctx, const tcr_storms *in, const TracksT<R> out, void *stream_, uint64_t *stats = nullptr,
                   const int64_t *stats_n_dev = nullptr, int64_t n_expected = 0)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    IntegrateWs &W = ctx->ws;
    const int64_t n = in->n;
    if (n < 0) return fail(ctx, "tcr_integrate: negative n");
    if (n == 0) return 0;
    const tcr_params &P = ctx->prm;
    const size_t ns = (size_t)P.n_steps;
    constexpr size_t REC = (size_t)step_rec_doubles<R>();
    if (W.d_fs.grow(ctx, ((size_t)n * ns * 4 * sizeof(R) + 7) / 8) < 0) return -1;
    const int max_rk = P.max_rk_steps > 0 ? P.max_rk_steps : 64;
    if (W.d_srec.grow(ctx, (size_t)n * max_rk * REC) < 0) return -1;
    if (max_rk > 65535) return fail(ctx, "tcr_params.max_rk_steps must be <= 65535");
    if (W.d_sidx.grow(ctx, ((size_t)n * ns * sizeof(uint16_t) + 7) / 8 * 4) < 0) return -1;     // [n][n_steps] uint16: step of each sample (whole doubles)
    R *fs = reinterpret_cast<R *>(W.d_fs.p);
    EvalKT<R> EK{};
    bool affine = false;
    if (eval_k_ready<R>(ctx, EK, &affine, st)) return -1;

    hipEvent_t *ev = nullptr;
    if (ctx->tr.timing && !ctx->capturing && timing_events(ctx, &ev)) return -1;
    if (ev) HIPCHK(ctx, hipEventRecord(ev[0], st));
    // Chain of launches with tail compaction (k_integrate): a pass parks the storms of waves that
    // fall under `thr` live lanes, the next pass needs at most waves*(thr-1)/64 waves for them.
    const int wps = std::is_same<R, double>::value ? TCR_INT_WPS : TCR_INT_WPS_F32;
    // (n_expected: how many of the n rows the caller expects to hold storms — a round's dense batch has capacity to spare)
    unsigned waves = integrate_waves(ctx, (n_expected > 0 && n_expected < n) ? n_expected : n, wps);
    const int thr = park_threshold(ctx, waves, wps);
    // With a chain, the forcing table is written in two segments: samples [0, 192) for every storm now, the rest after the
    // first pass and only for the storms that pass parks — the pass parks a storm (its lane takes the next one) as soon as
    // its next attempt could read beyond the first segment.  58 % of the storms never get there.
    // (only when the first pass is not also the last one: a last pass never parks, so a table cut at sample 191 would strand
    // every storm that lives beyond it — ADVICE r2: TCR_PARK forced on a batch of <= 8 waves)
    const unsigned final_waves = park_final_waves(ctx);
    const bool segmented = kFsMfmaColGroups == 2 && thr > 0 && waves > final_waves && kMaxPasses > 1 && fourier_on_matrix_cores(ctx) &&
                           (int)P.n_steps > kFsSegSamples + 16 && ctx->tune.table_segments != 0;
    // TC rows only: accept test 1 is decided in flight when 2 d is an output sample (KArgsT::prune_sample) — the integrator
    // appends the storms that pass to the TC list itself; otherwise k_screen decides it from the v part of the step records
    int prune_sample = -1;
    if (out.tc_rows_only && ctx->tune.prune != 0) {
        const double t2d = 2 * 86400.0, step_out = P.total_time / (double)(P.n_steps - 1);
        const int j = (int)floor(t2d / step_out);
        if (j >= 1 && j < P.n_steps - 1 && ts_host(P, j) == t2d) prune_sample = j;
    }
    const bool in_flight = prune_sample >= 0;
    // (a context that has used k_screen keeps its vrec when it changes to the in-flight path: freeing it here would need the
    // synchronisation and the re-capture of replayed rounds that an allocation needs)
    if (!in_flight && W.d_vrec.grow(ctx, (size_t)n * max_rk * kVRec) < 0) return -1;
    if (out.tc_rows_only && W.d_tc_idx.grow(ctx, (size_t)n) < 0) return -1;
    unsigned long long *tc_count = reinterpret_cast<unsigned long long *>(W.d_tc_count.p);
    {
        BatchReset z{};
        z.queue = W.d_queue.p; z.queue_words = (int)kQueueWords;
        if (in_flight) { z.flags = out.flags; z.n_flags = n; }
        if (out.tc_rows_only) z.tc_count = tc_count;
        if (launch_fourier<R>(ctx, n, in->n_dev, in->phases, fs, st, segmented ? kFsFirst : kFsAll, nullptr, nullptr, &z)) return -1;
    }
    STAGE(TCR_STAGE_FOURIER);
    if (ev) HIPCHK(ctx, hipEventRecord(ev[1], st));
    {
        KArgsT<R> a{};
        a.P = P; a.D = dev_fields(ctx); a.K = EK; a.n = n; a.n_dev = in->n_dev;
        a.lon0 = in->lon0; a.lat0 = in->lat0; a.v0 = in->v0; a.m0 = in->m0; a.h_bl = in->h_bl;
        a.slot = in->slot; a.phases = in->phases; a.fs = fs; a.srec = W.d_srec.p; a.vrec = in_flight ? nullptr : W.d_vrec.p; a.max_rk_steps = max_rk;
        a.n_valid = out.n_valid; a.status = out.status; a.nfev = out.nfev;
        a.n_accept = out.n_accept; a.n_reject = out.n_reject;
        a.queue = W.d_queue.p;
        a.prune_sample = prune_sample;
        if (in_flight) {
            // storms that pass accept test 1 go on the TC list as they end (flags of the others stay 0)
            a.tc_list = W.d_tc_idx.p; a.tc_count = tc_count;
        }
        // (the work queue / pass counters, the TC count and, with accept test 1 in flight, flags[] were zeroed by
        // the batch's first kernel — BatchReset; three hipMemsetAsync until round 4, which as captured memset nodes of a
        // replayed round did not reliably clear flags[]: tests/test_round.py)
        // (a segmented first pass can park any number of its storms)
        const size_t park_items = segmented ? (size_t)n : (size_t)waves * kWave;
        if (thr > 0 && W.d_park[0].grow(ctx, park_items * kParkRec) < 0) return -1;
        if (thr > 0 && W.d_park[1].grow(ctx, park_items * kParkRec) < 0) return -1;
        const bool probe = std::is_same<R, double>::value && W.d_probe;
        if (probe) { a.probe = W.d_probe; a.probe_cap = W.probe_cap; }
        bool seg_events = false;
        for (int pass = 0; pass < kMaxPasses; ++pass) {
            const bool last = thr <= 0 || waves <= final_waves || pass == kMaxPasses - 1;
            a.pass = pass;
            a.fill_pct = pass_fill_pct();
            a.threshold = last ? 0 : thr;
            a.park_in = W.d_park[(pass + 1) & 1].p;
            a.park_out = W.d_park[pass & 1].p;
            // the stage times of an attempt lie in [t, t_new] and the table lookup at t reads samples up to ceil(t / dt) + 1
            a.t_limit = (segmented && pass == 0) ? ts_host(P, kFsSegSamples - 2) : 1e300;
            launch_integrate(a, affine, probe, ctx->sg.static_mode, waves, st);
            if (last) break;
            if (segmented && pass == 0) {
                // the rest of the table, for the storms that are still alive (park list of pass 0, count on the device);
                // pass 1 may have as many storms as pass 0 had, so it keeps pass 0's waves
                if (ev) HIPCHK(ctx, hipEventRecord(ev[4], st));
                if (launch_fourier<R>(ctx, n, in->n_dev, in->phases, fs, st, kFsRest, W.d_park[0].p, W.d_queue.p + kMaxPasses)) return -1;
                if (ev) HIPCHK(ctx, hipEventRecord(ev[5], st));
                seg_events = true;
                continue;
            }
            waves = (unsigned)(((size_t)waves * (size_t)(thr - 1) + kWave - 1) / kWave);
        }
        if (ev && !seg_events) { HIPCHK(ctx, hipEventRecord(ev[4], st)); HIPCHK(ctx, hipEventRecord(ev[5], st)); }
    }
    STAGE(TCR_STAGE_INTEGRATE);
    // test instrument (tcr_integrate_steps_*_host): the records as k_integrate left them — K[7][4], before k_dense puts Q in its place
    if (W.d_steps) HIPCHK(ctx, hipMemcpyAsync(W.d_steps, W.d_srec.p, sizeof(double) * (size_t)n * max_rk * REC, hipMemcpyDeviceToDevice, st));
    if (ev) HIPCHK(ctx, hipEventRecord(ev[2], st));
    {
        EArgsT<R> a{};
        a.P = P; a.D = dev_fields(ctx); a.n = n; a.n_dev = in->n_dev; a.max_rk_steps = max_rk; a.srec = W.d_srec.p; a.vrec = in_flight ? nullptr : W.d_vrec.p; a.fs = fs;
        a.slot = in->slot; a.n_valid = out.n_valid; a.status = out.status; a.n_accept = out.n_accept;
        a.lon = out.lon; a.lat = out.lat; a.v = out.v; a.m = out.m; a.vmax = out.vmax;
        a.envw = out.envw; a.flags = out.flags; a.pad_state = out.pad_state;
        a.K = EK;
        const unsigned chunks = (unsigned)((ns + kPostThreads - 1) / kPostThreads);
        if (out.tc_rows_only) {
            // Only what the reference does (compute.py:185-204): accept test 1 from the v series alone, then env
            // winds, vmax and rows for the storms that passed.  The list stays on the device; the grids are
            // sized for the whole batch and workgroups beyond *count leave at once.
            if (!in_flight) {
                a.tc_list = W.d_tc_idx.p; a.tc_count = tc_count;
                hipLaunchKernelGGL(k_screen<R>, dim3((unsigned)((n + kScreenStorms - 1) / kScreenStorms)), dim3(kScreenThreads), 0, st, a);
            }
            // (in flight: the integrator has left the list already; the two stages stay in the trace, empty)
            STAGE(TCR_STAGE_SCREEN);
            STAGE(TCR_STAGE_SELECT_TC);          // (the list is k_screen's own since round 4: no compaction launch)
            a.list = W.d_tc_idx.p; a.count = W.d_tc_count.p;
        }
        // k_dense, TC rows only: a bounded grid of waves walks the device-side list (one wave per storm otherwise)
        int64_t cap = kEmitGridCap;
        if (ctx->tune.emit_grid_cap > 0) cap = ctx->tune.emit_grid_cap;     // tests: force several list entries per workgroup
        // (a batch of at most two grid caps gets a row of workgroups per storm: no overflow launch — a dispatch costs a small
        // batch more than 12 000 workgroups that find nothing to do)
        const unsigned gx = (out.tc_rows_only && n > 2 * cap) ? (unsigned)cap : (unsigned)n;
        hipLaunchKernelGGL(k_dense<R>, dim3(gx), dim3(kWave), 0, st, a, W.d_sidx.p);
        STAGE(TCR_STAGE_DENSE);
        // TC rows only: a bounded grid walks the device-side list (all rows: one row of workgroups per storm)
        const unsigned ex = gx;
        auto emit = [&](unsigned rows, bool overflow) {
            with_flags(affine, overflow, [&](auto A, auto OV) {
                hipLaunchKernelGGL((k_emit<R, decltype(A)::value, decltype(OV)::value>), dim3(rows, chunks), dim3(kPostThreads), 0, st, a, W.d_sidx.p);
            });
        };
        // list entries [0, ex): one per workgroup row, straight-line kernel; entries beyond the bounded grid (none
        // unless more than `cap` storms pass accept test 1; never with all rows, ex == n): a small grid that loops
        emit(ex, false);
        if ((int64_t)ex < n) {
            a.item_base = ex;
            emit((unsigned)std::min<int64_t>(n - ex, 256), true);
            a.item_base = 0;
        }
        STAGE(TCR_STAGE_EMIT);
        hipLaunchKernelGGL(k_flags<R>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, n, out.n_valid,
                           out.status, out.v, out.flags, out.pad_state, out.tc_rows_only ? 1 : 0, a.n_dev, out.nfev,
                           reinterpret_cast<unsigned long long *>(stats), stats_n_dev);
        STAGE(TCR_STAGE_FLAGS);
    }
    if (ev) HIPCHK(ctx, hipEventRecord(ev[3], st));
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// A batch's inputs from the caller's host arrays into B (the _host entry points): every storm's slot must be staged.
// need_m0 = false: m0 may be NULL (tcr_init_m_host computes it).
int storms_upload(tcr_ctx *ctx, DevBuf &B, const tcr_storms *in, tcr_storms *d, const char *who, bool need_m0 = true)
{
    const size_t n = (size_t)in->n;
    for (size_t i = 0; i < n; ++i)
        if (!slot_staged(ctx, in->slot[i])) return fail(ctx, "%s: storm references a slot that is not staged", who);
    *d = tcr_storms{};
    d->n = in->n;
    d->lon0 = B.put(in->lon0, n); d->lat0 = B.put(in->lat0, n); d->v0 = B.put(in->v0, n);
    d->m0 = (need_m0 || in->m0) ? B.put(in->m0, n) : nullptr;
    d->h_bl = B.put(in->h_bl, n); d->slot = B.put(in->slot, n);
    d->phases = B.put(in->phases, n * 4 * (size_t)ctx->prm.n_series);
    d->n_dev = nullptr;
    if (!d->lon0 || !d->lat0 || !d->v0 || ((need_m0 || in->m0) && !d->m0) || !d->h_bl || !d->slot || !d->phases)
        return fail(ctx, "%s: device allocation / upload failed", who);
    return 0;
}

template <typename R, typename T>
int integrate_host_impl(tcr_ctx *ctx, const tcr_storms *in, const T *out)
{
    if (ready(ctx, false)) return -1;
    if (!in || !out) return fail(ctx, "tcr_integrate_host: NULL argument");
    if (!enter(ctx)) return -1;
    const size_t n = (size_t)in->n, ns = (size_t)ctx->prm.n_steps;
    if (n == 0) return 0;
    DevBuf B;
    tcr_storms di{};
    if (storms_upload(ctx, B, in, &di, "tcr_integrate_host")) return -1;
    TracksT<R> dout{};
    dout.lon = B.get<R>(n * ns); dout.lat = B.get<R>(n * ns); dout.v = B.get<R>(n * ns);
    dout.m = B.get<R>(n * ns); dout.vmax = B.get<R>(n * ns); dout.envw = B.get<R>(n * ns * 4);
    dout.n_valid = B.get<int32_t>(n); dout.status = B.get<int32_t>(n); dout.flags = B.get<int32_t>(n);
    dout.nfev = B.get<int32_t>(n); dout.n_accept = B.get<int32_t>(n); dout.n_reject = B.get<int32_t>(n);
    if (!dout.lon || !dout.lat || !dout.v || !dout.m || !dout.vmax || !dout.envw || !dout.n_valid || !dout.status ||
        !dout.flags || !dout.nfev || !dout.n_accept || !dout.n_reject)
        return fail(ctx, "tcr_integrate_host: device allocation / upload failed");
    dout.tc_rows_only = 0;             // host buffers come back whole: every row is produced
    if (!std::is_same<R, double>::value && ensure_f32(ctx, ctx->stream)) return -1;
    if (integrate_impl<R>(ctx, &di, dout, ctx->stream)) return -1;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (d2h(ctx, out->lon, dout.lon, n * ns) || d2h(ctx, out->lat, dout.lat, n * ns) || d2h(ctx, out->v, dout.v, n * ns) ||
        d2h(ctx, out->m, dout.m, n * ns) || d2h(ctx, out->vmax, dout.vmax, n * ns) || d2h(ctx, out->envw, dout.envw, n * ns * 4) ||
        d2h(ctx, out->n_valid, dout.n_valid, n) || d2h(ctx, out->status, dout.status, n) || d2h(ctx, out->flags, dout.flags, n) ||
        d2h(ctx, out->nfev, dout.nfev, n) || d2h(ctx, out->n_accept, dout.n_accept, n) || d2h(ctx, out->n_reject, dout.n_reject, n))
        return -1;
    return 0;
}

// tcr_integrate_*_host plus the batch's accepted-step records (integrate_impl copies them while IntegrateWs::d_steps is set)
template <typename R, typename T>
int integrate_steps_impl(tcr_ctx *ctx, const char *who, const tcr_storms *in, const T *out, double *steps, int64_t steps_doubles)
{
    if (!ctx) return -1;
    if (!in || !out || !steps) return fail(ctx, "%s: NULL argument", who);
    if (ready(ctx, false)) return -1;
    if (ctx->ws.d_probe || ctx->ws.d_steps) return fail(ctx, "%s: another instrument of the integrator is active", who);
    if (!enter(ctx)) return -1;
    if (in->n <= 0) return 0;
    const int max_rk = ctx->prm.max_rk_steps > 0 ? ctx->prm.max_rk_steps : 64;
    const size_t need = (size_t)in->n * (size_t)max_rk * (size_t)step_rec_doubles<R>();
    if (steps_doubles < 0 || (size_t)steps_doubles != need)
        return fail(ctx, "%s: steps must hold n x max_rk_steps x step-record doubles (36 fp64, 20 fp32)", who);
    DevBuf B;
    double *d = B.get<double>(need);
    if (!d) return fail(ctx, "%s: device allocation failed", who);
    ctx->ws.d_steps = d;
    const int rc = integrate_host_impl<R>(ctx, in, out);
    ctx->ws.d_steps = nullptr;
    if (rc) return rc;
    HIPCHK(ctx, copy_sync(ctx->stream, steps, d, sizeof(double) * need, hipMemcpyDeviceToHost));
    return 0;
}

// R = float: the table and h_bl are rounded on the host, as k_integrate<float> gets them ((R) of the fp64 table value, (R)hb0)
template <typename R>
int probe_rhs_impl(tcr_ctx *ctx, const char *who, int slot, double h_bl, const double *Fs, int64_t n, const double *t,
                   const double *lon, const double *lat, const double *v, const double *m,
                   double *dydt, double *envw, double *alpha, double *aux)
{
    if (ready(ctx, false)) return -1;
    if (!enter(ctx)) return -1;
    if (!slot_staged(ctx, slot)) return fail(ctx, "%s: slot not staged", who);
    if (n <= 0) return 0;
    const size_t ns = (size_t)ctx->prm.n_steps;
    std::vector<R> fs(ns * 4);
    for (size_t i = 0; i < ns; ++i)
        for (int k = 0; k < 4; ++k) fs[i * 4 + k] = (R)Fs[(size_t)k * ns + i];
    DevBuf B;
    const R *d_fs = B.put(fs.data(), fs.size());
    const double *d_t = B.put(t, n), *d_lon = B.put(lon, n), *d_lat = B.put(lat, n), *d_v = B.put(v, n), *d_m = B.put(m, n);
    double *d_dy = B.get<double>(n * 4), *d_w = B.get<double>(n * 4), *d_al = B.get<double>(n);
    double *d_aux = aux ? B.get<double>(n * 24) : nullptr;
    if (!d_fs || !d_t || !d_lon || !d_lat || !d_v || !d_m || !d_dy || !d_w || !d_al || (aux && !d_aux))
        return fail(ctx, "%s: device allocation failed", who);
    if (!std::is_same<R, double>::value && ensure_f32(ctx, ctx->stream)) return -1;
    EvalKT<R> EK{};
    bool affine = false;
    if (eval_k_ready<R>(ctx, EK, &affine, ctx->stream)) return -1;
    const DevFields DF = dev_fields(ctx);
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    with_eval_variant(affine, ctx->sg.static_mode, [&](auto A, auto S) {
        hipLaunchKernelGGL((k_probe_rhs<R, decltype(A)::value, decltype(S)::value>), grid, block, 0, ctx->stream, ctx->prm, DF, EK, slot, (R)h_bl,
                           d_fs, n, d_t, d_lon, d_lat, d_v, d_m, d_dy, d_w, d_al, d_aux);
    });
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, copy_sync(ctx->stream, dydt, d_dy, sizeof(double) * n * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, copy_sync(ctx->stream, envw, d_w, sizeof(double) * n * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, copy_sync(ctx->stream, alpha, d_al, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (aux) HIPCHK(ctx, copy_sync(ctx->stream, aux, d_aux, sizeof(double) * n * 24, hipMemcpyDeviceToHost));
    return 0;
}

int init_m_launch(tcr_ctx *ctx, const tcr_storms *in, double dvdt, double *m_out, hipStream_t st)
{
    const DevFields DF = dev_fields(ctx);
    EvalK EK{};
    bool affine = false;
    if (eval_k_ready<double>(ctx, EK, &affine, st)) return -1;
    const dim3 grid((unsigned)((in->n + 63) / 64)), block(64);
    with_eval_variant(affine, ctx->sg.static_mode, [&](auto A, auto S) {
        hipLaunchKernelGGL((k_init_m<decltype(A)::value, decltype(S)::value>), grid, block, 0, st, ctx->prm, DF, EK, in->n, in->n_dev, in->lon0, in->lat0,
                           in->v0, in->m0, in->h_bl, in->slot, in->phases, dvdt, m_out);
    });
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int tcr_timing_enable(tcr_ctx *ctx, int on)
{
    if (!ctx) return -1;
    ctx->tr.timing = on != 0;
    ctx->tr.ev_used = 0;
    return 0;
}

int tcr_timing_sum(tcr_ctx *ctx, double ms[3], int64_t *n_calls)
{
    if (!ctx || !ms) return -1;
    Trace &T = ctx->tr;
    ms[0] = ms[1] = ms[2] = 0.0;
    const size_t calls = T.ev_used / kEvPerCall;
    if (n_calls) *n_calls = (int64_t)calls;
    if (!calls) return fail(ctx, "no timed launch recorded (tcr_timing_enable + tcr_integrate_*)");
    HIPCHK(ctx, hipEventSynchronize(T.ev_pool[T.ev_used - 1]));
    for (size_t c = 0; c < calls; ++c) {
        double one[3];
        if (timing_of_call(ctx, &T.ev_pool[c * kEvPerCall], one)) return -1;
        for (int i = 0; i < 3; ++i) ms[i] += one[i];
    }
    return 0;
}

int tcr_timing_last(tcr_ctx *ctx, double ms[3])
{
    if (!ctx || !ms) return -1;
    Trace &T = ctx->tr;
    if (T.ev_used < kEvPerCall) return fail(ctx, "no timed launch recorded (tcr_timing_enable + tcr_integrate_*)");
    hipEvent_t *q = &T.ev_pool[T.ev_used - kEvPerCall];
    HIPCHK(ctx, hipEventSynchronize(T.ev_pool[T.ev_used - 1]));
    return timing_of_call(ctx, q, ms);
}

int tcr_integrate_pass_stats(tcr_ctx *ctx, int64_t *out, int max_passes)
{
    if (!ctx || !out) return -1;
    if (!enter(ctx)) return -1;
    unsigned long long h[kQueueWords];
    HIPCHK(ctx, copy_sync(ctx->stream, h, ctx->ws.d_queue.p, sizeof(h), hipMemcpyDeviceToHost));
    int np = 0;
    for (int p = 0; p < kMaxPasses && p < max_passes; ++p) {
        if (h[2 * kMaxPasses + 4 * p] == 0 && h[p] == 0) break;
        out[6 * p + 0] = (int64_t)h[p];                               // items requested from the queue (>= items)
        out[6 * p + 1] = (int64_t)h[kMaxPasses + p];                  // storms parked for the next pass
        out[6 * p + 2] = (int64_t)h[2 * kMaxPasses + 4 * p + 0];      // wave cycles
        out[6 * p + 3] = (int64_t)h[2 * kMaxPasses + 4 * p + 1];      // live-lane cycles
        out[6 * p + 4] = (int64_t)h[2 * kMaxPasses + 4 * p + 2];      // wave wall-clock ticks (100 MHz)
        out[6 * p + 5] = (int64_t)h[2 * kMaxPasses + 4 * p + 3];      // wave shader-clock ticks
        ++np;
    }
    return np;
}

int tcr_sync(tcr_ctx *ctx, void *stream)
{
    if (!ctx) return -1;
    HIPCHK(ctx, hipStreamSynchronize(stream ? (hipStream_t)stream : ctx->stream));
    return 0;
}

int tcr_integrate_dev(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks *out, void *stream_)
{
    if (ready(ctx, false)) return -1;
    if (!in || !out) return fail(ctx, "tcr_integrate_dev: NULL argument");
    if (ctx->ws.d_steps) return fail(ctx, "the step records are an instrument of the host entry points");
    return integrate_impl<double>(ctx, in, tracks_of<double>(out), stream_);
}

int tcr_integrate_f32_dev(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks_f32 *out, void *stream_)
{
    if (ready(ctx, false)) return -1;
    if (!in || !out) return fail(ctx, "tcr_integrate_f32_dev: NULL argument");
    if (ctx->ws.d_probe) return fail(ctx, "the decision probe is an fp64 instrument");
    if (ctx->ws.d_steps) return fail(ctx, "the step records are an instrument of the host entry points");
    hipStream_t st = enter(ctx, stream_);
    if (!st || ensure_f32(ctx, st)) return -1;
    return integrate_impl<float>(ctx, in, tracks_of<float>(out), stream_);
}

int tcr_integrate_host(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks *out)
{
    return integrate_host_impl<double>(ctx, in, out);
}

int tcr_integrate_f32_host(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks_f32 *out)
{
    if (ctx && ctx->ws.d_probe) return fail(ctx, "the decision probe is an fp64 instrument");
    return integrate_host_impl<float>(ctx, in, out);
}

int tcr_integrate_probe_host(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks *out, uint8_t *dec, int32_t cap)
{
    if (!ctx) return -1;
    if (!in || !dec || cap <= 0) return fail(ctx, "tcr_integrate_probe_host: bad argument");
    if (!enter(ctx)) return -1;
    if (in->n <= 0) return 0;
    DevBuf B;
    const size_t bytes = (size_t)in->n * (size_t)cap;
    uint8_t *d = B.get<uint8_t>(bytes);
    if (!d) return fail(ctx, "tcr_integrate_probe_host: device allocation failed");
    HIPCHK(ctx, hipMemsetAsync(d, 0xff, bytes, ctx->stream)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->ws.d_probe = d; ctx->ws.probe_cap = cap;
    const int rc = tcr_integrate_host(ctx, in, out);
    ctx->ws.d_probe = nullptr; ctx->ws.probe_cap = 0;
    if (rc) return rc;
    HIPCHK(ctx, copy_sync(ctx->stream, dec, d, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int tcr_integrate_steps_host(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks *out, double *steps, int64_t steps_doubles)
{
    return integrate_steps_impl<double>(ctx, "tcr_integrate_steps_host", in, out, steps, steps_doubles);
}

int tcr_integrate_steps_f32_host(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks_f32 *out, double *steps, int64_t steps_doubles)
{
    return integrate_steps_impl<float>(ctx, "tcr_integrate_steps_f32_host", in, out, steps, steps_doubles);
}

int tcr_fourier_table_host(tcr_ctx *ctx, int64_t n, const double *phases, double *Fs)
{
    if (!ctx) return -1;
    if (!ctx->have_prm) return fail(ctx, "tcr_params_set has not been called");
    if (!enter(ctx)) return -1;
    if (n <= 0) return 0;
    const size_t ns = (size_t)ctx->prm.n_steps, N = (size_t)ctx->prm.n_series;
    DevBuf B;
    const double *d_ph = B.put(phases, (size_t)n * 4 * N);
    double *d_fs = B.get<double>((size_t)n * ns * 4);
    if (!d_ph || !d_fs) return fail(ctx, "tcr_fourier_table_host: device allocation failed");
    if (launch_fourier(ctx, n, nullptr, d_ph, d_fs, ctx->stream)) return -1;
    std::vector<double> h((size_t)n * ns * 4);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), d_fs, sizeof(double) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // device layout [n][n_steps][4] -> reference layout [n][4][n_steps]
    for (int64_t s = 0; s < n; ++s)
        for (size_t i = 0; i < ns; ++i)
            for (int k = 0; k < 4; ++k) Fs[((size_t)s * 4 + k) * ns + i] = h[((size_t)s * ns + i) * 4 + k];
    return 0;
}

int tcr_probe_math_host(tcr_ctx *ctx, int32_t fn, int64_t n, const double *a, const double *b, double *out)
{
    if (!ctx) return -1;
    if (fn < 0 || fn > 12 || n < 0 || (n > 0 && (!a || !out)) || ((fn == 0 || fn == 6) && n > 0 && !b)) return fail(ctx, "tcr_probe_math_host: bad argument");
    if (n == 0) return 0;
    if (!enter(ctx)) return -1;
    DevBuf B;
    const double *d_a = B.put(a, n), *d_b = b ? B.put(b, n) : nullptr;
    double *d_o = B.get<double>(n);
    if (!d_a || (b && !d_b) || !d_o) return fail(ctx, "tcr_probe_math_host: device allocation failed");
    if (fn <= 5) hipLaunchKernelGGL(k_probe_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)fn, n, d_a, d_b, d_o);
    else hipLaunchKernelGGL(k_probe_math_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)fn, n, d_a, d_b, d_o);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, copy_sync(ctx->stream, out, d_o, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

int tcr_probe_rhs_host(tcr_ctx *ctx, int slot, double h_bl, const double *Fs, int64_t n, const double *t,
                       const double *lon, const double *lat, const double *v, const double *m,
                       double *dydt, double *envw, double *alpha)
{
    return probe_rhs_impl<double>(ctx, "tcr_probe_rhs_host", slot, h_bl, Fs, n, t, lon, lat, v, m, dydt, envw, alpha, nullptr);
}

int tcr_probe_rhs_f32_host(tcr_ctx *ctx, int slot, double h_bl, const double *Fs, int64_t n, const double *t,
                           const double *lon, const double *lat, const double *v, const double *m,
                           double *dydt, double *envw, double *alpha, double *aux)
{
    return probe_rhs_impl<float>(ctx, "tcr_probe_rhs_f32_host", slot, h_bl, Fs, n, t, lon, lat, v, m, dydt, envw, alpha, aux);
}

int tcr_init_m_dev(tcr_ctx *ctx, const tcr_storms *in, double dvdt, double *m_out_dev, void *stream_)
{
    if (ready(ctx, false)) return -1;
    if (!in || !m_out_dev || !in->lon0 || !in->lat0 || !in->v0 || !in->h_bl || !in->slot || !in->phases)
        return fail(ctx, "tcr_init_m_dev: NULL argument");
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    if (in->n <= 0) return 0;
    return init_m_launch(ctx, in, dvdt, m_out_dev, st);
}

int tcr_init_m_host(tcr_ctx *ctx, const tcr_storms *in, double dvdt, double *m_out)
{
    if (ready(ctx, false)) return -1;
    if (!in || !m_out || !in->lon0 || !in->lat0 || !in->v0 || !in->h_bl || !in->slot || !in->phases)
        return fail(ctx, "tcr_init_m_host: NULL argument");
    if (!enter(ctx)) return -1;
    const int64_t n = in->n;
    if (n <= 0) return 0;
    DevBuf B;
    tcr_storms d{};
    if (storms_upload(ctx, B, in, &d, "tcr_init_m_host", false)) return -1;
    double *d_out = B.get<double>(n);
    if (!d_out) return fail(ctx, "tcr_init_m_host: device allocation / upload failed");
    if (init_m_launch(ctx, &d, dvdt, d_out, ctx->stream)) return -1;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, copy_sync(ctx->stream, m_out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
