// The context behind the C ABI: what a tcr_ctx owns, grouped by the host file that works on it — staging (tcr_stage.hip), the
// integrator's workspaces (tcr_integrate.hip), the round and its graphs (tcr_round.hip), timing and stage trace, the analyses
// (tcr_hazard.hip ... tcr_climatology.hip).  Every member owns what it points to (tcr_host.h): there is no list of frees.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

#include "tcr_host.h"
#include "tcr_seed.hip"                    // RoundKey

namespace {

struct GridStore {
    std::vector<double> lon, lat;
    DevArray<double> d_lon, d_lat, d_rlon, d_rlat;
    bool affine_lon = false, affine_lat = false;
    bool set = false;
    // fp32 view of the same grid (built on first use of an fp32 entry point): knots rounded to float,
    // reciprocal widths and the affine test redone in float arithmetic
    std::vector<float> lon32, lat32;
    DevArray<float> d_lon32, d_lat32, d_rlon32, d_rlat32;
    bool affine_lon32 = false, affine_lat32 = false;
    bool set32 = false;
};

struct SlotStore {
    DevArray<double> wind, thermo, rh;
    DevArray<float> wind32, thermo32;           // fp32 copies (tcr_integrate_f32_*), converted on the device
    bool f32_stale = true;
};

// Host threads that copy a month slot's planes from the caller's (pageable) arrays into the pinned staging buffer: one
// thread moves ~10 GB/s, a slot of the global basin is 9.9 MB and crosses PCIe in 0.2 ms — the copy into pinned memory, not
// the link, is what a year's staging waits for.  Fork / join per call; the caller takes part.
struct CopyPool {
    struct Seg { char *dst; const char *src; size_t bytes; };
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    const Seg *segs = nullptr;
    size_t n_segs = 0;
    std::atomic<size_t> next{0};
    int active = 0;
    uint64_t gen = 0;
    bool stop = false;

    explicit CopyPool(int helpers)
    {
        for (int i = 0; i < helpers; ++i) th.emplace_back([this] { loop(); });
    }
    ~CopyPool()
    {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv_go.notify_all();
        for (auto &t : th) t.join();
    }
    void work()
    {
        for (size_t i; (i = next.fetch_add(1)) < n_segs;) memcpy(segs[i].dst, segs[i].src, segs[i].bytes);
    }
    void loop()
    {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
            }
            work();
            std::lock_guard<std::mutex> lk(mu);
            if (--active == 0) cv_done.notify_one();
        }
    }
    void run(const std::vector<Seg> &v)
    {
        if (v.empty()) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            segs = v.data(); n_segs = v.size(); next = 0; active = (int)th.size(); ++gen;
        }
        cv_go.notify_all();
        work();
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return active == 0; });
    }
};

// The blocks of ScanWs::d: records, caps (storms, then segments), record counts, partial counts, chunk table + pair counter, the
// prep kernel's own, two of the analysis's own.
enum { kWsRec, kWsCaps, kWsCnt, kWsPart, kWsTab, kWsPrep, kWsOwn0, kWsOwn1, kWsBlocks };

// Workspace of one site-scan analysis (tcr_sitescan.h), blocks in bytes.  h: the pinned staging of the chunk table.
struct ScanWs {
    DevArray<char> d[kWsBlocks];
    PinnedArray<int64_t> h;
    hipEvent_t ev = nullptr, done = nullptr;        // chunk table uploaded / last call done
    unsigned long long *pairs = nullptr;            // pairs the last call evaluated (inside d[kWsTab])
    ~ScanWs() { destroy_events(&ev, 1); destroy_events(&done, 1); }
};

// Fields in HBM (interleaved layouts of tcr_device.h) and the way they get there: tcr_stage.hip
struct Staging {
    GridStore wg, tg, hg, bg, mg, rg;           // wind, thermo, land (+ bathymetry when shared), bathymetry (when on its own grid), masks, rh
    std::vector<SlotStore> slots;
    DevArray<tcr::DevSlot> d_slots;
    bool slots_dirty = true;
    DevArray<double> d_stat;                    // [lat][lon][2] land, bathymetry interleaved (one shared grid)
    DevArray<double> d_land, d_bathy;           // separate planes when the two grids differ (split_static)
    DevArray<float> d_stat32, d_land32, d_bathy32;      // fp32 copies of the land / bathymetry planes
    bool stat32_stale = true;
    bool split_static = false;                  // land and bathymetry on two grids (hg, bg)
    // exact narrow storage of the two (tcr_device.h, StaticMode): kStatPack16 -> d_nstat = uint16 [lat][lon];
    // kStatU8F32 -> d_nstat = the uint8 land plane, d_nbathy = the float bathymetry plane
    int static_mode = tcr::kStatF64;
    int static_pref = 0;                        // tcr_static_store: 0 auto, 1 fp64 planes
    DevArray<uint8_t> d_nstat;                  // (bytes, whatever the mode's element is)
    DevArray<float> d_nbathy;
    size_t static_bytes = 0;                    // footprint of the staged land + bathymetry
    DevArray<uint8_t> d_mask_bits;              // the eight mask planes as the bits of one byte per grid point
    DevArray<double> d_tab;                     // entropy table: p[np], s[ns], T[np][ns]
    int tab_np = 0, tab_ns = 0;
    // field staging: two pinned halves (the host fills one while the interleave kernel reads the other over the link); nothing
    // waits on the host until the fields are used (fields_pending)
    PinnedArray<double> h_stage[2];             // (cap: doubles per half)
    hipEvent_t h_stage_ev[2] = {nullptr, nullptr};
    int h_stage_next = 0;
    bool fields_pending = false;
    double stage_ms[5] = {0, 0, 0, 0, 0};       // host time of the slot uploads: wait for the pinned half, copy, enqueue transfer, enqueue kernel; [4] calls
    std::unique_ptr<CopyPool> pool;
    ~Staging() { destroy_events(h_stage_ev, 2); }
};

// Grow-only workspaces of a batch (forcing tables, track records, queues): tcr_integrate.hip
struct IntegrateWs {
    DevArray<double> d_fs, d_srec;              // forcing tables, accepted-step records
    DevArray<double> d_vrec;                    // the v part of the step records, packed (k_integrate -> k_screen; only when k_screen runs)
    DevArray<unsigned long long> d_queue;       // work-queue heads and parked-storm counts of k_integrate's passes
    DevArray<uint16_t> d_sidx;                  // sample -> accepted-step map (k_dense -> k_emit)
    DevArray<double> d_park[2];                 // ping-pong lists of parked storms
    DevArray<double2> d_sc_table;               // one period of (sin, cos)(2π j / period)
    DevArray<double2> d_pf;                     // weighted phase factors [n][n_series][4] of the periodic Fourier kernel
    int fs_period = 0;                          // 0: direct Fourier kernel
    DevArray<int32_t> d_tc_idx;                 // storms that passed accept test 1 (k_integrate or k_screen -> k_dense / k_emit), tc_rows_only
    DevArray<int64_t> d_tc_count;
    uint8_t *d_probe = nullptr;                 // decision probe of the next tcr_integrate_dev (tcr_integrate_probe_host; that call's DevBuf owns it)
    int probe_cap = 0;
    double *d_steps = nullptr;                  // where the next batch's step records are copied before k_dense rewrites them (tcr_integrate_steps_*_host; that call's DevBuf owns it)
};

struct RoundGraph { std::vector<uint8_t> key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; bool failed = false; };

// Scratch of a round's selection stages and the rounds replayed from captured graphs (tcr_round_dev): the device copy of the
// round key the replayed kernels read, and the graphs keyed by the bytes of their descriptor and the epoch (tcr_host.h): tcr_round.hip
struct RoundState {
    DevArray<unsigned long long> d_tiles;       // scratch of k_compact: ticket, generation, one word per tile (zeroed when allocated)
    DevArray<int32_t> d_cell; int cell_bins = 0;        // scratch of tcr_cell_order_dev
    bool cell_counts_open = false;              // a compaction that counts cells has been enqueued, the rank kernel that zeroes them again not yet
    DevArray<unsigned int> d_hist_partial;      // k_seed_hist: per-workgroup counts + ticket (zero between launches)
    DevArray<tcr::RoundKey> d_round_key;
    std::vector<RoundGraph> graphs;
    int64_t n_replays = 0;
    void drop_graphs()
    {
        for (auto &g : graphs) { if (g.exec) (void)hipGraphExecDestroy(g.exec); if (g.graph) (void)hipGraphDestroy(g.graph); }
        graphs.clear();
    }
    ~RoundState() { drop_graphs(); }
};

struct Trace {
    // timing: kEvPerCall events per timed tcr_integrate_dev call since tcr_timing_enable(ctx, 1)
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    // stage trace (tcr_stage_trace_enable): one event behind every stage of a directly enqueued round
    bool stage_trace = false;
    std::vector<hipEvent_t> st_pool;
    std::vector<int> st_id;
    size_t st_used = 0;
    ~Trace() { destroy_events(ev_pool.data(), ev_pool.size()); destroy_events(st_pool.data(), st_pool.size()); }
};

struct Analyses {
    // site hazard (tcr_hazard.hip), wind footprint (tcr_windfield.hip), portfolio loss (tcr_loss.hip), rainfall
    // (tcr_rainfall.hip), compound hazard (tcr_compound.hip), wind duration (tcr_duration.hip), rain accumulation windows
    // (tcr_accumulation.hip), directional wind (tcr_directional.hip) and closest approach (tcr_approach.hip): a workspace each, so
    // that one call of each may be in flight on streams of their own
    ScanWs hz, wf, ls, rf, cp, du, ac, dr, ca;
    // landfall (tcr_landfall.hip): node coordinates (lon, then lat) and land bit plane of the uploaded grid
    DevArray<double> lf_xy;
    DevArray<uint32_t> lf_bits;
    int64_t lf_nlon = 0, lf_nlat = 0;
    bool lf_periodic = false;
    double lf_guess[4] = {0, 0, 0, 0};              // lon0, (nlon - 1) / lon span, lat0, (nlat - 1) / lat span
    // track climatology (tcr_climatology.hip): key workspace of tracks longer than the kernel's LDS slice
    DevArray<uint64_t> d_cl;
};

}  // namespace

struct tcr_ctx : HostCtx {
    tcr_params prm;
    bool have_prm = false;
    int cu_count = 256;
    int storms_per_lane = 1;                    // tcr_schedule_set
    tcr_tune tune;                              // launch-shape knobs: the environment at tcr_ctx_create, then tcr_tune_set
    Staging sg;
    IntegrateWs ws;
    RoundState rd;
    Trace tr;
    Analyses an;
};
