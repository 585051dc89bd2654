// A round of the accept loop: seeding, compaction, cell order, gather, stats, pack, seed histogram as entry points of their
// own, everything a round enqueues (enqueue_round), tcr_round_dev with its cache of captured graphs, and the stage trace.
#pragma once
#include <cstddef>

#include "tcr_integrate.hip"

namespace {

int seed_impl(tcr_ctx *ctx, uint64_t experiment_seed, int32_t year, int64_t cand0, const RoundKey *key,
              const tcr_seeds *out, void *stream_)
{
    if (ready(ctx, true)) return -1;
    if (!out) return fail(ctx, "tcr_seed_dev: NULL argument");
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    if (out->n <= 0) return 0;
    for (auto &s : ctx->sg.slots) if (!s.rh.p) return fail(ctx, "tcr_seed_dev: a slot has no rh_mid (tcr_rh_upload)");
    if (!ctx->sg.rg.set) return fail(ctx, "tcr_seed_dev: rh_mid not staged (tcr_rh_upload)");
    if (ctx->sg.slots.size() < 12) return fail(ctx, "tcr_seed_dev: needs the 12 month slots staged");
    SeedArgs a{};
    a.P = ctx->prm; a.D = dev_fields(ctx); a.seed = experiment_seed; a.year = year; a.cand0 = cand0; a.out = *out; a.key = key;
    hipLaunchKernelGGL(k_seed, dim3((unsigned)((out->n + 255) / 256)), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// cell != NULL: the selection's cell keys and counts are produced on the way (k_compact<true>), for cell_order_impl(key_done)
int compact_impl(tcr_ctx *ctx, int64_t n, const int32_t *flags, int32_t mask, int64_t max_out,
                 int32_t *idx, int64_t *count, void *stream_, const CellOrderArgs *cell)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    if (!flags || !idx || !count || n < 0 || max_out < 0) return fail(ctx, "tcr_compact_dev: bad argument");
    DevArray<unsigned long long> &tw = ctx->rd.d_tiles;
    const int64_t tiles = std::max<int64_t>(1, (n + kScanTile - 1) / kScanTile);       // (n == 0: one tile writes *count = 0)
    const int grown = tw.grow(ctx, (size_t)tiles + 2, 1022);
    if (grown < 0) return -1;
    if (grown) HIPCHK(ctx, hipMemsetAsync(tw.p, 0, sizeof(unsigned long long) * tw.cap, st));
    if (cell) hipLaunchKernelGGL(k_compact<true>, dim3((unsigned)tiles), dim3(kScanThreads), 0, st, n, flags, mask, max_out, idx, count, tw.p, (int)tiles, *cell);
    else hipLaunchKernelGGL(k_compact<false>, dim3((unsigned)tiles), dim3(kScanThreads), 0, st, n, flags, mask, max_out, idx, count, tw.p, (int)tiles, CellOrderArgs{});
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// scratch and arguments of the locality order of idx[0 .. min(n, *count))
int cell_order_args(tcr_ctx *ctx, const tcr_seeds *cand, int32_t *idx, int64_t n, const int64_t *count, double cell_deg,
                    hipStream_t st, CellOrderArgs &a)
{
    RoundState &S = ctx->rd;
    if (!cand || !cand->lon0 || !cand->lat0 || !idx || n < 0) return fail(ctx, "tcr_cell_order_dev: bad argument");
    if (!(cell_deg >= 0.25 && cell_deg <= 90.0)) return fail(ctx, "tcr_cell_order_dev: cell_deg must be in [0.25, 90]");
    a = CellOrderArgs{};
    a.ncol = (int)ceil(360.0 / cell_deg);
    const int nrow = (int)ceil(180.0 / cell_deg) + 1;
    a.nbins = a.ncol * nrow;
    if (a.nbins > (1 << 20)) return fail(ctx, "tcr_cell_order_dev: too many cells");
    // scratch (int32): cell counters [nbins + 1] (zero between calls: k_cell_rank leaves them so), offsets [nbins + 1], the list
    // of long cells [nbins + 2], then idx copy [n], key [n], tmp [n], tmp_key [n]
    const size_t head = 3 * ((size_t)a.nbins + 1) + 8;
    const size_t words = head + 4 * (size_t)n;
    const int grown = S.d_cell.grow(ctx, (words + 1) / 2 * 2, 8192);          // (an even number of words: whole doubles)
    if (grown < 0) return -1;
    if (grown || S.cell_bins != a.nbins) {
        HIPCHK(ctx, hipMemsetAsync(S.d_cell.p, 0, sizeof(int32_t) * head, st));
        S.cell_bins = a.nbins;
        S.cell_counts_open = false;
    } else if (S.cell_counts_open && !ctx->capturing) {
        // an earlier ordering was abandoned between the kernel that counts the cells and the one that leaves the counters zero
        // (an enqueue error in between): the counters are not relied on, they are cleared
        HIPCHK(ctx, hipMemsetAsync(S.d_cell.p, 0, sizeof(int32_t) * head, st));
        S.cell_counts_open = false;
    }
    int32_t *w = S.d_cell.p;
    a.hist = w; a.start = w + a.nbins + 1; a.long_cells = w + 2 * (a.nbins + 1);
    int32_t *body = w + head;
    a.idx_in = body; a.key = body + n; a.tmp = body + 2 * n; a.tmp_key = body + 3 * n;
    a.lon0 = cand->lon0; a.lat0 = cand->lat0; a.idx_out = idx; a.count = count; a.n = n;
    a.inv_cell = 1.0 / cell_deg;
    return 0;
}

// key_done: the keys and cell counts came with the compaction (k_compact<true>)
int cell_order_launch(tcr_ctx *ctx, const CellOrderArgs &a, bool key_done, hipStream_t st)
{
    const int64_t n = a.n;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    ctx->rd.cell_counts_open = true;
    if (!key_done) hipLaunchKernelGGL(k_cell_key, dim3(blocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_cell_scan, dim3(1), dim3(kCellScanThreads), 0, st, a);
    hipLaunchKernelGGL(k_cell_scatter, dim3(blocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_cell_rank, dim3((unsigned)((std::max<int64_t>(n, a.nbins + 1) + 255) / 256)), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    ctx->rd.cell_counts_open = false;              // k_cell_rank leaves the counters zero
    return 0;
}

int gather_impl(tcr_ctx *ctx, const tcr_seeds *src, const int32_t *idx, int64_t n_out, const int64_t *count,
                const tcr_seeds *dst, uint64_t experiment_seed, int32_t year, int64_t cand0, const RoundKey *key, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    if (!ctx->have_prm) return fail(ctx, "tcr_params_set has not been called");
    if (!src || !dst || !idx) return fail(ctx, "tcr_gather_seeds_dev: NULL argument");
    if (n_out <= 0) return 0;
    GatherSeedArgs a{};
    a.src = *src; a.dst = *dst; a.idx = idx; a.n_out = n_out; a.phases_per_storm = 4 * ctx->prm.n_series;
    a.seed = experiment_seed; a.year = year; a.cand0 = cand0; a.count = count; a.key = key;
    const int64_t threads = n_out * kGatherLanes;
    hipLaunchKernelGGL(k_gather_seeds, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

template <typename R, typename T>
int pack_impl(tcr_ctx *ctx, const T *src, const int32_t *idx, const int64_t *count, int64_t cap, double *packed,
              int64_t row_stride, void *stream_, const int32_t *cand_idx = nullptr, const int32_t *slot = nullptr,
              const int32_t *basin_idx = nullptr, int64_t cand0 = 0, const RoundKey *key = nullptr)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    if (!ctx->have_prm) return fail(ctx, "tcr_params_set has not been called");
    if (!src || !idx || !count || !packed) return fail(ctx, "tcr_pack_tracks: NULL argument");
    if (cap <= 0) return 0;
    PackArgsT<R> a{};
    a.lon = src->lon; a.lat = src->lat; a.v = src->v; a.m = src->m; a.vmax = src->vmax; a.envw = src->envw;
    a.idx = idx; a.count = count; a.cap = cap; a.ns = ctx->prm.n_steps; a.packed = packed;
    a.row_stride = row_stride > 0 ? row_stride : 9 * (int64_t)ctx->prm.n_steps;
    if (a.row_stride < 9 * (int64_t)ctx->prm.n_steps) return fail(ctx, "tcr_pack_tracks: row_stride < 9 * n_steps");
    if (slot) {
        if (!basin_idx) return fail(ctx, "tcr_pack_tracks_meta_dev: slot and basin_idx go together");
        if (a.row_stride < 9 * (int64_t)ctx->prm.n_steps + 3) return fail(ctx, "tcr_pack_tracks_meta_dev: row_stride < 9 * n_steps + 3");
        a.cand_idx = cand_idx; a.slot = slot; a.basin_idx = basin_idx; a.cand0 = cand0; a.key = key;
    }
    hipLaunchKernelGGL(k_pack_tracks<R>, dim3((unsigned)cap), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int seed_hist_impl(tcr_ctx *ctx, const tcr_seeds *cand, int64_t n, int64_t cand0, const RoundKey *key, const double *cutoff,
                   int64_t *out, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    if (!cand || !cand->seed_flags || !cand->basin_idx || !cand->slot || !out) return fail(ctx, "tcr_seed_hist_dev: NULL argument");
    SeedHistArgs a{};
    a.seed_flags = cand->seed_flags; a.basin_idx = cand->basin_idx; a.slot = cand->slot; a.n = n > 0 ? n : 0; a.cand0 = cand0;
    a.key = key; a.cutoff = cutoff; a.out = reinterpret_cast<unsigned long long *>(out);
    const size_t words = (size_t)kSeedHistBlocks * TCR_N_BASINS * 12 + 16;
    const int grown = ctx->rd.d_hist_partial.grow(ctx, words);
    if (grown < 0) return -1;
    if (grown) HIPCHK(ctx, hipMemsetAsync(ctx->rd.d_hist_partial.p, 0, sizeof(unsigned int) * words, st));
    a.partial = ctx->rd.d_hist_partial.p;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(kSeedHistBlocks, (a.n + 1023) / 1024));
    hipLaunchKernelGGL(k_seed_hist, dim3((unsigned)blocks), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// Everything a round enqueues (see tcr_round_dev in the header).  key != NULL: the replayable form — seed / year / cand0
// are read on the device.
int enqueue_round(tcr_ctx *ctx, const tcr_round *r, uint64_t seed, int32_t year, int64_t cand0, const RoundKey *key, void *st)
{
    tcr_seeds cand = r->cand, storms = r->storms;
    cand.n = r->n_cand; storms.n = r->n_storms;
    STAGE(TCR_STAGE_START);
    if (seed_impl(ctx, seed, year, cand0, key, &cand, st)) return -1;
    STAGE(TCR_STAGE_SEED);
#ifdef TCR_EXPERIMENTS
    tcr_exp::dummy_launches((hipStream_t)st, reinterpret_cast<unsigned long long *>(ctx->rd.d_cell.p));
#endif
    if (r->cell_deg > 0) {
        // locality order: with many cells the keys and cell counts are produced by the compaction itself (one launch less)
        CellOrderArgs ca{};
        if (cell_order_args(ctx, &cand, r->cand_idx, r->n_storms, r->n_passed, r->cell_deg, (hipStream_t)st, ca)) return -1;
        const bool fused = ca.nbins > kCellLdsBins;
        if (fused) ctx->rd.cell_counts_open = true;
        if (compact_impl(ctx, r->n_cand, cand.seed_flags, 2, r->n_storms, r->cand_idx, r->n_passed, st, fused ? &ca : nullptr)) return -1;
        STAGE(TCR_STAGE_SELECT);
        if (cell_order_launch(ctx, ca, fused, (hipStream_t)st)) return -1;
    } else {
        if (compact_impl(ctx, r->n_cand, cand.seed_flags, 2, r->n_storms, r->cand_idx, r->n_passed, st, nullptr)) return -1;
        STAGE(TCR_STAGE_SELECT);
    }
    STAGE(TCR_STAGE_ORDER);
    if (gather_impl(ctx, &cand, r->cand_idx, r->n_storms, r->n_passed, &storms, seed, year, cand0, key, st)) return -1;
    STAGE(TCR_STAGE_GATHER);
    tcr_storms in{};
    in.n = r->n_storms; in.lon0 = storms.lon0; in.lat0 = storms.lat0; in.v0 = storms.v0; in.m0 = storms.m0; in.h_bl = storms.h_bl;
    in.slot = storms.slot; in.phases = storms.phases; in.n_dev = r->exact_count ? r->n_passed : nullptr;
    if (r->f32) {
        if (ensure_f32(ctx, (hipStream_t)st)) return -1;
        if (integrate_impl<float>(ctx, &in, tracks_of<float>(reinterpret_cast<const tcr_tracks_f32 *>(&r->tracks)), st, r->stats, r->n_passed, r->n_expected)) return -1;
    } else if (integrate_impl<double>(ctx, &in, tracks_of<double>(&r->tracks), st, r->stats, r->n_passed, r->n_expected)) return -1;
    // (the stats of tcr_stats_dev are accumulated by the batch's last kernel, k_flags)
    STAGE(TCR_STAGE_STATS);
    if (r->acc_idx) {
        if (!r->n_accepted) return fail(ctx, "tcr_round_dev: acc_idx without n_accepted");
        if (compact_impl(ctx, r->n_storms, r->tracks.flags, TCR_FLAG_ACCEPTED, r->n_storms, r->acc_idx, r->n_accepted, st, nullptr)) return -1;
        if (r->packed && r->pack_cap > 0) {
            // the meta columns go with a record that has room for them (pack_stride >= 9 * n_steps + 3)
            const bool meta = r->pack_stride >= 9 * (int64_t)ctx->prm.n_steps + 3;
            const int32_t *ci = meta ? r->cand_idx : nullptr, *sl = meta ? storms.slot : nullptr, *bi = meta ? storms.basin_idx : nullptr;
            if (r->f32 ? pack_impl<float>(ctx, reinterpret_cast<const tcr_tracks_f32 *>(&r->tracks), r->acc_idx, r->n_accepted, r->pack_cap,
                                          r->packed, r->pack_stride, st, ci, sl, bi, cand0, key)
                       : pack_impl<double>(ctx, &r->tracks, r->acc_idx, r->n_accepted, r->pack_cap, r->packed, r->pack_stride, st,
                                           ci, sl, bi, cand0, key)) return -1;
        }
    }
    if (r->seed_hist && seed_hist_impl(ctx, &cand, r->n_cand, cand0, key, nullptr, r->seed_hist, st)) return -1;
    STAGE(TCR_STAGE_PACK);
    return 0;
}

}  // namespace

extern "C" {

int tcr_seed_dev(tcr_ctx *ctx, uint64_t experiment_seed, int32_t year, int64_t cand0,
                 const tcr_seeds *out, void *stream_)
{
    return seed_impl(ctx, experiment_seed, year, cand0, nullptr, out, stream_);
}

int tcr_seed_host(tcr_ctx *ctx, uint64_t experiment_seed, int32_t year, int64_t cand0, const tcr_seeds *out)
{
    if (ready(ctx, true)) return -1;
    if (!out) return fail(ctx, "tcr_seed_host: NULL argument");
    if (!enter(ctx)) return -1;
    const size_t n = (size_t)out->n, N = (size_t)ctx->prm.n_series;
    if (n == 0) return 0;
    DevBuf B;
    tcr_seeds d{};
    d.n = out->n;
    d.lon0 = B.get<double>(n); d.lat0 = B.get<double>(n); d.v0 = B.get<double>(n); d.m0 = B.get<double>(n);
    d.h_bl = B.get<double>(n); d.slot = B.get<int32_t>(n); d.phases = B.get<double>(n * 4 * N);
    d.basin_idx = B.get<int32_t>(n); d.seed_flags = B.get<int32_t>(n);
    if (!d.lon0 || !d.lat0 || !d.v0 || !d.m0 || !d.h_bl || !d.slot || !d.phases || !d.basin_idx || !d.seed_flags)
        return fail(ctx, "tcr_seed_host: device allocation failed");
    if (tcr_seed_dev(ctx, experiment_seed, year, cand0, &d, ctx->stream)) return -1;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (d2h(ctx, out->lon0, d.lon0, n) || d2h(ctx, out->lat0, d.lat0, n) || d2h(ctx, out->v0, d.v0, n) || d2h(ctx, out->m0, d.m0, n) ||
        d2h(ctx, out->h_bl, d.h_bl, n) || d2h(ctx, out->slot, d.slot, n) || d2h(ctx, out->phases, d.phases, n * 4 * N) ||
        d2h(ctx, out->basin_idx, d.basin_idx, n) || d2h(ctx, out->seed_flags, d.seed_flags, n))
        return -1;
    return 0;
}

int tcr_compact_dev(tcr_ctx *ctx, int64_t n, const int32_t *flags, int32_t mask, int64_t max_out,
                    int32_t *idx, int64_t *count, void *stream_)
{
    return compact_impl(ctx, n, flags, mask, max_out, idx, count, stream_, nullptr);
}

int tcr_cell_order_dev(tcr_ctx *ctx, const tcr_seeds *cand, int32_t *idx, int64_t n, const int64_t *count,
                       double cell_deg, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    CellOrderArgs a{};
    if (cell_order_args(ctx, cand, idx, n, count, cell_deg, st, a)) return -1;
    if (n == 0) return 0;
    return cell_order_launch(ctx, a, false, st);
}

int tcr_gather_seeds_dev(tcr_ctx *ctx, const tcr_seeds *src, const int32_t *idx, int64_t n_out,
                         const int64_t *count, const tcr_seeds *dst, uint64_t experiment_seed, int32_t year,
                         int64_t cand0, void *stream_)
{
    return gather_impl(ctx, src, idx, n_out, count, dst, experiment_seed, year, cand0, nullptr, stream_);
}

int tcr_stats_dev(tcr_ctx *ctx, int64_t n, const int64_t *n_dev, const tcr_tracks *t, uint64_t *out, int32_t n_out, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    if (!t || !out) return fail(ctx, "tcr_stats_dev: NULL argument");
    if (n_out != 6 && n_out != 8 && n_out != TCR_N_STATS) return fail(ctx, "tcr_stats_dev: n_out must be 6, 8 or 10 (the capacity of out_dev in words)");
    if (n <= 0) return 0;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 512) blocks = 512;
    hipLaunchKernelGGL(k_stats, dim3((unsigned)blocks), dim3(256), 0, st, n, n_dev, t->n_valid, t->nfev, t->flags, t->status,
                       reinterpret_cast<unsigned long long *>(out), (int)n_out);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int tcr_pack_tracks_dev(tcr_ctx *ctx, const tcr_tracks *src, const int32_t *idx, const int64_t *count,
                        int64_t cap, double *packed, int64_t row_stride, void *stream_)
{
    return pack_impl<double>(ctx, src, idx, count, cap, packed, row_stride, stream_);
}

int tcr_pack_tracks_f32_dev(tcr_ctx *ctx, const tcr_tracks_f32 *src, const int32_t *idx, const int64_t *count,
                            int64_t cap, double *packed, int64_t row_stride, void *stream_)
{
    return pack_impl<float>(ctx, src, idx, count, cap, packed, row_stride, stream_);
}

int tcr_pack_tracks_meta_dev(tcr_ctx *ctx, const tcr_tracks *src, int32_t f32, const int32_t *idx, const int64_t *count,
                             int64_t cap, double *packed, int64_t row_stride, const int32_t *cand_idx, const int32_t *slot,
                             const int32_t *basin_idx, int64_t cand0, void *stream_)
{
    if (ctx && (!slot || !basin_idx)) return fail(ctx, "tcr_pack_tracks_meta_dev: NULL argument");
    if (f32) return pack_impl<float>(ctx, reinterpret_cast<const tcr_tracks_f32 *>(src), idx, count, cap, packed, row_stride, stream_,
                                     cand_idx, slot, basin_idx, cand0);
    return pack_impl<double>(ctx, src, idx, count, cap, packed, row_stride, stream_, cand_idx, slot, basin_idx, cand0);
}

int tcr_seed_hist_dev(tcr_ctx *ctx, const tcr_seeds *cand, int64_t cand0, const double *cutoff, int64_t *out, void *stream_)
{
    return seed_hist_impl(ctx, cand, cand ? cand->n : 0, cand0, nullptr, cutoff, out, stream_);
}

int tcr_round_dev(tcr_ctx *ctx, const tcr_round *r, uint64_t seed, int32_t year, int64_t cand0, int32_t use_graph, void *stream_)
{
    if (ready(ctx, true)) return -1;
    if (!r) return fail(ctx, "tcr_round_dev: NULL argument");
    if (r->n_cand <= 0 || r->n_storms <= 0) return fail(ctx, "tcr_round_dev: n_cand and n_storms must be positive");
    if (r->n_storms > r->n_cand) return fail(ctx, "tcr_round_dev: n_storms > n_cand");
    if (!r->cand_idx || !r->n_passed || !r->cand.seed_flags || !r->cand.lon0 || !r->storms.lon0 || !r->storms.phases ||
        !r->storms.basin_idx || !r->tracks.flags || !r->tracks.n_valid)
        return fail(ctx, "tcr_round_dev: NULL buffer");
    if (r->cell_deg != 0 && !(r->cell_deg >= 0.25 && r->cell_deg <= 90.0)) return fail(ctx, "tcr_round_dev: cell_deg must be 0 or in [0.25, 90]");
    if (ctx->ws.d_steps) return fail(ctx, "the step records are an instrument of the host entry points");
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    if (!use_graph || ctx->ws.d_probe) return enqueue_round(ctx, r, seed, year, cand0, nullptr, st);

    // ---- replayed form
    RoundState &S = ctx->rd;
    std::vector<uint8_t> key(sizeof(tcr_round) + sizeof(uint64_t) + sizeof(void *));
    memcpy(key.data(), r, sizeof(tcr_round));
    {   // the one run of padding bytes in the descriptor (behind tcr_tracks.tc_rows_only) must not take part in the comparison
        constexpr size_t pad0 = offsetof(tcr_round, tracks) + offsetof(tcr_tracks, tc_rows_only) + sizeof(int32_t);
        constexpr size_t pad1 = offsetof(tcr_round, tracks) + sizeof(tcr_tracks);
        static_assert(pad1 >= pad0 && sizeof(tcr_seeds) == 80 && sizeof(tcr_round) == 384, "tcr_round layout changed: revisit the key");
        memset(key.data() + pad0, 0, pad1 - pad0);
    }
    memcpy(key.data() + sizeof(tcr_round), &ctx->epoch, sizeof(uint64_t));
    memcpy(key.data() + sizeof(tcr_round) + sizeof(uint64_t), &st, sizeof(void *));
    RoundGraph *g = nullptr;
    for (auto &c : S.graphs) if (c.key == key) { g = &c; break; }
    if (!g) {
        // First sight of this descriptor (or the context has allocated / changed parameters since): run the round directly
        // — that is this call's result and it sizes every workspace — then capture the same enqueue for the calls to come.
        if (!S.graphs.empty() && memcmp(S.graphs.front().key.data() + sizeof(tcr_round), &ctx->epoch, sizeof(uint64_t)) != 0)
            S.drop_graphs();                     // graphs of an older epoch hold stale addresses
        if (S.graphs.size() >= 64) S.drop_graphs();           // a caller that keeps changing its buffers: start over rather than grow
        if (enqueue_round(ctx, r, seed, year, cand0, nullptr, st)) return -1;
        memcpy(key.data() + sizeof(tcr_round), &ctx->epoch, sizeof(uint64_t));     // the direct run may have grown workspaces
        S.graphs.emplace_back();
        g = &S.graphs.back();
        g->key = key;
        // Capture.  HIP's capture state is fragile against the rest of the process: a legacy-stream operation on ANY thread
        // while this stream captures (a synchronous hipMemcpy of another context's field upload, say) fails there with
        // "would make the legacy stream depend on a capturing blocking stream" and invalidates the capture here.  Whatever
        // happens, the stream must leave capture mode and the sticky error must be cleared; the descriptor then keeps the
        // direct form (this call's round has already run).
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { g->failed = true; (void)hipGetLastError(); return 0; }
        ctx->capturing = true;
        const int rc = enqueue_round(ctx, r, 0, 0, 0, S.d_round_key.p, st);
        ctx->capturing = false;
        hipGraph_t graph = nullptr;
        hipError_t e = hipStreamEndCapture(st, &graph);
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
            hipGraph_t junk = nullptr;                      // still (invalidly) capturing: end it once more
            (void)hipStreamEndCapture(st, &junk);
            if (junk) (void)hipGraphDestroy(junk);
            e = hipErrorStreamCaptureInvalidated;
        }
        for (int k = 0; k < 4 && hipGetLastError() != hipSuccess; ++k) {}
        if (rc || e != hipSuccess || !graph) {
            if (graph) (void)hipGraphDestroy(graph);
            ctx->err.clear();
            g->failed = true;                    // this descriptor keeps the direct form; the round above has run
            return 0;
        }
#ifdef TCR_EXPERIMENTS
        tcr_exp::graph_dot(graph);
#endif
        hipGraphExec_t exec = nullptr;
        if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess || !exec) {
            (void)hipGraphDestroy(graph); (void)hipGetLastError();
            g->failed = true;
            return 0;
        }
        g->graph = graph; g->exec = exec;
        return 0;
    }
    if (g->failed) return enqueue_round(ctx, r, seed, year, cand0, nullptr, st);
    // (the fp32 copies of re-staged fields are refreshed here: the captured enqueue found them up to date and holds no conversion)
    if (r->f32 && ensure_f32(ctx, st)) return -1;
    hipLaunchKernelGGL(k_set_round_key, dim3(1), dim3(1), 0, st, S.d_round_key.p, seed, year, cand0);
    HIPCHK(ctx, hipGraphLaunch(g->exec, st));
    ++S.n_replays;
    return 0;
}

int tcr_stage_trace_enable(tcr_ctx *ctx, int on)
{
    if (!ctx) return -1;
    ctx->tr.stage_trace = on != 0;
    ctx->tr.st_used = 0;
    return 0;
}

int tcr_stage_trace_sum(tcr_ctx *ctx, double ms[TCR_N_STAGES], int64_t *n_rounds)
{
    if (!ctx || !ms) return -1;
    Trace &T = ctx->tr;
    for (int i = 0; i < TCR_N_STAGES; ++i) ms[i] = 0.0;
    int64_t rounds = 0;
    if (T.st_used) HIPCHK(ctx, hipEventSynchronize(T.st_pool[T.st_used - 1]));
    for (size_t i = 0; i < T.st_used; ++i) {
        const int id = T.st_id[i];
        if (id == TCR_STAGE_START) { ++rounds; continue; }
        if (i == 0 || id < 0 || id >= TCR_N_STAGES) continue;
        float f = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&f, T.st_pool[i - 1], T.st_pool[i]));
        ms[id] += f;
    }
    if (n_rounds) *n_rounds = rounds;
    return 0;
}

int tcr_round_graph_stats(tcr_ctx *ctx, int64_t *n_graphs, int64_t *n_replays)
{
    if (!ctx) return -1;
    int64_t n = 0;
    for (auto &g : ctx->rd.graphs) n += g.exec ? 1 : 0;
    if (n_graphs) *n_graphs = n;
    if (n_replays) *n_replays = ctx->rd.n_replays;
    return 0;
}

}  // extern "C"
