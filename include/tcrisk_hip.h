/*
 * tcrisk_hip.h — C ABI of libtcrisk_hip.so, the MI355X (gfx950) implementation of
 * the per-storm hot path of linjonathan/tropical_cyclone_risk.
 *
 * The reference has no FFI: the seam it exposes is the Python method boundary
 *     Coupled_FAST.init_fields / .gen_track / ._env_winds   (intensity/coupled_fast.py:217-267,
 *                                                            track/bam_track.py:116-128)
 * driven once per candidate seed by util/compute.py:run_tracks (compute.py:134-209).
 * This ABI is the *batched* form of that seam: fields are staged once per
 * (month) slot, then whole batches of storms are integrated per call.  Every
 * entry point cites the reference interface it replaces.
 *
 * Conventions
 *   - plain C types only; the caller owns every buffer it passes;
 *   - functions return 0 on success, <0 on error (tcr_last_error() has the text);
 *   - "host" pointers are ordinary memory, "dev" pointers are HIP device memory
 *     (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void*
 *     (NULL = the context's own stream);
 *   - all floating point is IEEE fp64 (the reference computes in fp64 throughout);
 *   - 2-D planes are [lat][lon] row-major with lat ascending, already cropped to
 *     the basin box exactly as TC_Basin.transform_global_field does
 *     (util/basins.py:57-75): lookups clamp to the cropped grid's edge like
 *     RectBivariateSpline(kx=1,ky=1).ev.
 */
#ifndef TCRISK_HIP_H
#define TCRISK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCR_ABI_VERSION 7
#define TCR_NW 4            /* ua250, va250, ua850, va850  (track/env_wind.py:22-26) */
#define TCR_NCOV 10         /* packed lower triangle (0,0),(1,0),(1,1),(2,0)..(3,3) (env_wind.py:31-42) */
#define TCR_MAX_SERIES 32
#define TCR_N_BASINS 7      /* sorted ids AU,EP,NA,NI,SI,SP,WP (util/compute.py:87) */

/* per-storm status (gen_track's return, intensity/coupled_fast.py:229-267) */
#define TCR_STATUS_GATED (-1)      /* ventilation gate: gen_track returned None (coupled_fast.py:238-244) */
#define TCR_STATUS_FINISHED 0      /* solve_ivp status 0: reached total_time */
#define TCR_STATUS_EVENT 1         /* solve_ivp status 1: tc_dissipates fired (coupled_fast.py:246-256) */
#define TCR_STATUS_STEP_FAIL (-2)  /* solve_ivp status -1: step size underflow */
#define TCR_STATUS_STEP_OVERFLOW (-3) /* more accepted RK steps than tcr_params.max_rk_steps: raise it */

/* flags bit field written by the post-step (util/compute.py:185-209) */
#define TCR_FLAG_IS_TC 1           /* any(v >= 15) and v(2 d) >= 6.5        (compute.py:185-189) */
#define TCR_FLAG_ACCEPTED 2        /* ... and nanmax(vmax) >= 18            (compute.py:205)     */

typedef struct tcr_ctx tcr_ctx;

/* 1-D coordinate pair of a rectilinear grid (strictly increasing, may be non-uniform) */
typedef struct {
    int32_t nlon, nlat;
    const double *lon;      /* host, [nlon] */
    const double *lat;      /* host, [nlat] */
} tcr_grid;

/* namelist scalars the path reads (namelist.py:56-94) + solve_ivp options
 * (coupled_fast.py:264-266) + Coupled_FAST constants (coupled_fast.py:23-27). */
typedef struct {
    double Ck, epsilon, kappa;              /* namelist.py:57; coupled_fast.py:25-26 */
    double u_beta, v_beta;                  /* namelist.py:77-78 */
    double T_Fs;                            /* namelist.T_days * 86400 (bam_track.py:56) */
    double y_alpha[2], m_alpha[2], alpha_max[2], alpha_min[2];   /* namelist.py:73-76 */
    double steering_coefs[2];               /* namelist.py:71 (used when !coupled_track) */
    double dt_out, total_time;              /* namelist.py:48-49 */
    double rtol, atol, max_step;            /* solve_ivp defaults + coupled_fast.py:266 */
    double v_thresh, v_2d_thresh, vmax_thresh;   /* namelist.py:81-83 */
    double v_dissipate;                     /* 4 m/s (coupled_fast.py:255) */
    double earth_R;                         /* util/constants.py:7 */
    double box[4];                          /* basin lon_min, lat_min, lon_max, lat_max (basins.py:42-50) */
    double fs_amp;                          /* sqrt(2 / sum(n^-3)), computed by the host with NumPy */
    double fs_wgt[TCR_MAX_SERIES];          /* n^-1.5 */
    int32_t n_series;                       /* 15 (bam_track.py:112) */
    int32_t n_steps;                        /* int(total_time/dt_out)+1 (bam_track.py:54) */
    int32_t coupled_track;                  /* namelist.py:72 */
    int32_t max_rk_steps;                   /* capacity of the per-storm accepted-step record (0 = 64) */
    /* seeding (util/compute.py:134-175) */
    double seed_v_init;                     /* namelist.py:80 */
    double pi_gate;                         /* 35 m/s (compute.py:168) */
    double lat_vort_fac;                    /* namelist.py:88 */
    double lat_vort_power[TCR_N_BASINS];    /* namelist.py:89-92, sorted-id order */
    double atm_bl_depth[TCR_N_BASINS];      /* namelist.py:85-86, sorted-id order */
    double minit_a, minit_b, minit_c, minit_d;   /* f_mInit = a/(1+exp(-(rh-b)*c))+d (namelist.py:94) */
} tcr_params;

/* A batch of storms; every pointer is [n] unless noted.  Used with host or
 * device memory depending on the entry point. */
typedef struct {
    int64_t n;
    const double *lon0, *lat0, *v0, *m0;    /* gen_track(clon, clat, v, m)  (coupled_fast.py:229) */
    const double *h_bl;                     /* fast.h_bl = atm_bl_depth[basin] (compute.py:175) */
    const int32_t *slot;                    /* field slot = genesis month - 1 (compute.py:151-152) */
    const double *phases;                   /* [n][4][n_series] uniforms of gen_f (bam_track.py:27) */
    /* Optional device scalar (tcr_integrate_dev only; NULL otherwise): only the first min(n, *n_dev) storms
     * exist — the count tcr_compact_dev left on the device — so a round of the accept loop needs no host
     * synchronisation between seeding and integration.  Grids are sized for n; flags of the rows beyond are 0. */
    const int64_t *n_dev;
} tcr_storms;

/* Outputs: the per-storm part of run_tracks' 9-tuple (compute.py:124-133, 210) */
typedef struct {
    double *lon, *lat, *v, *m, *vmax;       /* [n][n_steps], NaN after the track end */
    double *envw;                           /* [n][n_steps][4] (tc_env_wnds) */
    int32_t *n_valid;                       /* emitted samples (len(res.t)) */
    int32_t *status;                        /* TCR_STATUS_* */
    int32_t *flags;                         /* TCR_FLAG_* */
    int32_t *nfev;                          /* RHS evaluations (res.nfev) */
    int32_t *n_accept, *n_reject;           /* accepted steps / rejected attempts */
    /* Optional (may be NULL), [n]: padding state of the plane rows.  The NaN padding is 2/3 of
     * the plane bytes; a caller that reuses the same plane buffers batch after batch passes this
     * array with them, initialised to -1 ("unknown").  On entry pad_state[r] = k >= 0 promises
     * that row r of every plane is already NaN from sample k on, so only [n_valid, k) needs
     * re-padding; on return pad_state[r] = n_valid[r].  The planes come out bit-identical to a
     * full padding.  NULL or -1: the whole tail is written. */
    int32_t *pad_state;
    /* 0: rows are produced for every storm of the batch (what the parity tests compare).
     * 1: rows are produced only where the reference produces them — for candidates that pass accept test 1
     *    (`if is_tc:`, compute.py:190-204): env winds, vmax and the row writes are skipped for the others
     *    (~90 % of a batch); their rows and pad_state entries are left untouched (unspecified contents).
     *    n_valid, status, flags, nfev, n_accept, n_reject are complete in both modes, and the rows of
     *    is_tc storms are bit-identical in both.  tcr_integrate_host always produces every row. */
    int32_t tc_rows_only;
} tcr_tracks;

/* The same outputs in fp32 (BASELINE config 5, "fp32 intensity ODE"): float planes, same layout and meaning. */
typedef struct {
    float *lon, *lat, *v, *m, *vmax;        /* [n][n_steps], NaN after the track end */
    float *envw;                            /* [n][n_steps][4] */
    int32_t *n_valid, *status, *flags, *nfev, *n_accept, *n_reject;
    int32_t *pad_state;
    int32_t tc_rows_only;
} tcr_tracks_f32;

/* ---- lifecycle ----------------------------------------------------------- */
int tcr_abi_version(void);
/* replaces: constructing the 12 Coupled_FAST objects of a year (compute.py:119) */
int tcr_ctx_create(int device, tcr_ctx **out);
int tcr_ctx_destroy(tcr_ctx *ctx);
/* last error text of a context (ctx == NULL: of the last failed tcr_ctx_create) */
const char *tcr_last_error(const tcr_ctx *ctx);

/* replaces: `import namelist` reads scattered through the path */
int tcr_params_set(tcr_ctx *ctx, const tcr_params *p);

/* ---- field staging (once per experiment / year) --------------------------- */
/* replaces: geo.read_bathy / geo.read_land (intensity/geo.py:9-34, coupled_fast.py:30-31) */
int tcr_static_upload(tcr_ctx *ctx, const tcr_grid *hg, const double *land, const double *bathy);
/* the same with the land mask and the bathymetry each on its own grid, as the two independent interpolators
 * f_land / f_bath of the reference allow (intensity/geo.py:9-34); equal grids take the one-grid path */
int tcr_static_upload2(tcr_ctx *ctx, const tcr_grid *land_grid, const double *land,
                       const tcr_grid *bathy_grid, const double *bathy);
/* How the two planes are kept in HBM.  The reference hands float64 arrays to RectBivariateSpline whatever the files hold
 * (intensity/geo.py:15-19, 29-33) — its own land.nc is int8 0 / 1 on a 0.125-degree grid (1440 x 2880).  With pref 0 (auto,
 * the default) an upload inspects the VALUES and stores them narrow when that is exact: land 0 / 1 and whole-metre
 * bathymetry in [-16384, 16383] on one grid -> one uint16 per grid point (mode 2); land in 0 .. 255 and a bathymetry that
 * round-trips through float32 -> eight bytes per grid point on one grid (mode 4), a uint8 and a float plane on two (mode 3);
 * anything else the fp64 planes of pref 1 (mode 0, or 1
 * on two grids).  The kernels widen to the same doubles before any arithmetic, so results do not depend on the mode.
 * Call before tcr_static_upload*.  tcr_static_info reports the mode in use and the bytes the planes occupy.
 * A context may be re-staged with other planes (the mode is chosen again) — not while launches that read them are in flight. */
int tcr_static_store(tcr_ctx *ctx, int32_t pref);
int tcr_static_info(tcr_ctx *ctx, int32_t *mode, int64_t *bytes);
/* replaces: BetaAdvectionTrack._load_wnd_stat (bam_track.py:76-91) +
 *           Coupled_FAST.init_fields (coupled_fast.py:217-225) for one month slot.
 */
int tcr_fields_upload(tcr_ctx *ctx, int slot,
                      const tcr_grid *wg, const double *const mean[TCR_NW], const double *const cov[TCR_NCOV],
                      const tcr_grid *tg, const double *vpot, const double *chi,
                      const double *mld, const double *strat);
/* replaces: m_init_fx[month] = mat.interp2_fx(lon, lat, rh_mid_month) (compute.py:111): mid-level
 * RH of one month slot on the *uncropped* thermo grid, as the reference builds it; only the
 * device-side seeding reads it (initial m, compute.py:173-174). */
int tcr_rh_upload(tcr_ctx *ctx, int slot, const tcr_grid *rg, const double *rh_mid);
/* tcr_fields_upload + tcr_rh_upload of one month slot in ONE transfer (rg / rh_mid may both be NULL).  All three calls copy
 * the planes into pinned memory (tcr_tune.copy_threads host threads), enqueue one asynchronous transfer and the device kernel
 * that interleaves the planes into the slot's layouts, and return: the caller's arrays are free again, and the library waits
 * for the staged fields when they are first used.  Do not stage a slot while launches that read it are still in flight. */
int tcr_slot_upload(tcr_ctx *ctx, int slot,
                    const tcr_grid *wg, const double *const mean[TCR_NW], const double *const cov[TCR_NCOV],
                    const tcr_grid *tg, const double *vpot, const double *chi, const double *mld, const double *strat,
                    const tcr_grid *rg, const double *rh_mid);
/* measurement: host milliseconds the slot uploads of this context have spent since the last reset — [0] waiting for the pinned
 * half a transfer two slots back was still reading, [1] copying planes into pinned memory, [2] enqueuing the transfer,
 * [3] enqueuing the interleave kernel — and [4] the number of uploads */
int tcr_stage_timing(tcr_ctx *ctx, double ms[5], int32_t reset);
/* replaces: the land/<B>.nc interpolators f_b and f_basins (compute.py:87-97).
 * masks are uint8 0/1 planes on one global grid; run_mask is the run basin's. */
int tcr_masks_upload(tcr_ctx *ctx, const tcr_grid *mg, const uint8_t *run_mask,
                     const uint8_t *const basin_masks[TCR_N_BASINS]);

/* ---- the hot path ---------------------------------------------------------- */
/* replaces: the per-candidate body of run_tracks — gen_track (compute.py:176),
 * accept test 1 (:185-189), env-wind recompute (:201-202), axi_to_max_wind
 * (:203-204), accept test 2 (:205) — for a whole batch.  Host buffers. */
int tcr_integrate_host(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks *out);
/* same with device buffers, asynchronous on `stream`.  Results do not depend on how the library schedules a batch
 * (tcr_tune below; tests/test_gpu_parity.py::test_full_size_ensemble_properties). */
int tcr_integrate_dev(tcr_ctx *ctx, const tcr_storms *in_dev, const tcr_tracks *out_dev, void *stream);

/* Launch shape of batches that do not fill the chip (fewer than 64 storms per SIMD).  The reference has no counterpart: it
 * integrates one storm at a time.  storms_per_lane = 1 (default): one integrator lane per storm, the shortest time to a
 * single batch's results (its longest storm's ~300 sequential evaluations).  k > 1: n / (64 k) persistent waves whose lanes
 * take ~k storms in turn from the batch's queue — about a third of the SIMD time per batch at k = 4 for a ~1.4x longer
 * chain, which is what a caller with many batches in flight on other streams / contexts wants (bench.py, pipelined years).
 * Results do not depend on it. */
int tcr_schedule_set(tcr_ctx *ctx, int32_t storms_per_lane);

/* Launch-shape knobs of a context (the reference has no counterpart).  Results never depend on them.  A context starts from
 * the environment — TCR_WAVES, TCR_PARK, TCR_PARK_FINAL, TCR_TABLE_SEGMENTS, TCR_PRUNE, TCR_EMIT_GRID_CAP, TCR_COPY_THREADS,
 * read ONCE, in tcr_ctx_create; no entry point reads the environment afterwards — and tcr_tune_set replaces all of them.
 * A negative field = the library's own choice. */
typedef struct {
    int32_t waves;            /* persistent integrator waves per launch (default: from the batch size and tcr_schedule_set) */
    int32_t park;             /* tail-compaction threshold of k_integrate's chain of passes; 0 = one launch (default: 12 when a
                                 launch fills the chip, else 0) */
    int32_t park_final;       /* a pass of at most this many waves runs to the end (default 8) */
    int32_t table_segments;   /* 0: the forcing table in one piece instead of a second segment written only for the storms the
                                 first integration pass parks (default 1) */
    int32_t prune;            /* tc_rows_only: 0 = accept test 1 by a kernel of its own over every storm (k_screen, from the v
                                 part of the step records); otherwise (default 1) decided in flight by the integrator, which
                                 lists the storms that pass — when 2 d is an output sample, else as 0 */
    int32_t emit_grid_cap;    /* workgroup rows walking the list of storms that pass accept test 1 (default 8192) */
    int32_t copy_threads;     /* host threads that copy a month slot's planes into the pinned staging buffer (default 4) */
    int32_t table_factors;    /* 0: the forcing table's phase factors by a kernel of their own (k_phase_factors_frag, fragments in
                                 HBM); otherwise (default 1) formed inside the table kernel from the phases */
} tcr_tune;
int tcr_tune_set(tcr_ctx *ctx, const tcr_tune *t);
int tcr_tune_get(tcr_ctx *ctx, tcr_tune *t);

/* The fp32 variant of the same path (BASELINE config 5; the reference itself is fp64 throughout, so this is a
 * documented departure with a stated tolerance, see DESIGN.md and profiles/r02_fp32_study.json): fields are
 * converted to fp32 on the device on first use, state / stage derivatives / right-hand side / dense output are
 * fp32, rows come out as fp32; time, the output grid and the step-size controller (error norm, accept test,
 * step factor) stay fp64.  Storm inputs are the same fp64 tcr_storms.  Device buffers, asynchronous on `stream`. */
int tcr_integrate_f32_dev(tcr_ctx *ctx, const tcr_storms *in_dev, const tcr_tracks_f32 *out_dev, void *stream);
int tcr_integrate_f32_host(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks_f32 *out);

/* replaces: the rejection-sampling seed loop (compute.py:134-175) for candidates
 * [cand0, cand0+n) of `year`, drawn from Philox4x32-10 keyed by
 * (experiment_seed, year, candidate index).  Device buffers (all [n]):
 * lon0, lat0, v0, m0, h_bl, slot, phases as tcr_storms; basin_idx (sorted-id
 * index), seed_flags bit0 = counts toward n_seeds (compute.py:165-167),
 * bit1 = passed the PI gate (compute.py:168).  phases may be NULL (see tcr_gather_seeds_dev). */
typedef struct {
    int64_t n;
    double *lon0, *lat0, *v0, *m0, *h_bl;
    int32_t *slot;
    double *phases;
    int32_t *basin_idx;
    int32_t *seed_flags;
} tcr_seeds;
int tcr_seed_dev(tcr_ctx *ctx, uint64_t experiment_seed, int32_t year, int64_t cand0,
                 const tcr_seeds *out_dev, void *stream);
int tcr_seed_host(tcr_ctx *ctx, uint64_t experiment_seed, int32_t year, int64_t cand0,
                  const tcr_seeds *out_host);

/* ---- order-preserving filters (the batched form of the sequential accept loop) -- */
/* replaces: `while not seed_passed` / `if is_tc` / `nt += 1` control flow of run_tracks
 * (compute.py:135-209): indices i in [0,n) with (flags[i] & mask) != 0, in increasing
 * order, first max_out of them -> idx; *count = how many matched (device scalar). */
int tcr_compact_dev(tcr_ctx *ctx, int64_t n, const int32_t *flags_dev, int32_t mask, int64_t max_out,
                    int32_t *idx_dev, int64_t *count_dev, void *stream);
/* Locality order of a selection (no reference counterpart: the reference integrates one storm at a time): reorders
 * idx_dev[0 .. min(n, *count_dev)) — candidate indices as tcr_compact_dev leaves them — by the cell_deg-degree cell of
 * the candidates' genesis points (latitude row major, stable: candidate order within a cell), so that the storms
 * tcr_gather_seeds_dev then places next to each other, and the integrator runs in one wave, read the same parts of the
 * fields.  Per-storm results do not depend on the order of a batch; a caller that needs candidate order (the accept loop
 * of run_tracks) sorts the few accepted rows back by their candidate index.  Cells that hold many entries (large cells over
 * a small basin; NaN positions, which all sort into cell 0) are sorted as segments, so the worst case stays O(n log^2 n).
 * Like every entry point it works in scratch owned by the context: one stream per context at a time.  (The scan kernel
 * holds 66 KB of LDS: gfx950-class parts.) */
int tcr_cell_order_dev(tcr_ctx *ctx, const tcr_seeds *cand_dev, int32_t *idx_dev, int64_t n, const int64_t *count_dev,
                       double cell_deg, void *stream);
/* dense storm batch dst[r] = src[idx[r]], r < min(n_out, *count_dev) (count_dev, the device scalar
 * written by tcr_compact_dev, may be NULL = all n_out rows are valid).  If src_dev->phases is NULL (tcr_seed_dev was
 * asked not to write them: most candidates never pass) the 4*n_series Fourier phases of the selected
 * candidates are drawn here from the same Philox stream (candidate = cand0 + idx[r]). */
int tcr_gather_seeds_dev(tcr_ctx *ctx, const tcr_seeds *src_dev, const int32_t *idx_dev, int64_t n_out,
                         const int64_t *count_dev, const tcr_seeds *dst_dev, uint64_t experiment_seed,
                         int32_t year, int64_t cand0, void *stream);
/* sums over a finished batch, for throughput accounting and round control: out_dev[0] = storm-steps
 * (sum of max(n_valid-1, 0)), [1] = RHS evaluations, [2] = output samples, [3] = accepted tracks,
 * [4] = storms that passed accept test 1 (is_tc), [5] = output samples of those storms (the rows
 * tc_rows_only produces), [6] = 1 if *n_dev < n (the batch was short of storms: a round control signal that
 * needs no host round trip), [7] = storms counted (min(n, *n_dev)), [8] = storms whose step record overflowed
 * (status TCR_STATUS_STEP_OVERFLOW), [9] = storms the batch had no room for (max(*n_dev - n, 0): passing seeds that
 * tcr_compact_dev clipped).  The counters are uint64 and are ADDED to (zero them first).  n_out is the capacity of
 * out_dev in words — 6, 8 or 10 (TCR_N_STATS): only counters below it are written (ABI v5; v4 wrote eight through an
 * unsized pointer). */
#define TCR_N_STATS 10
int tcr_stats_dev(tcr_ctx *ctx, int64_t n, const int64_t *n_dev, const tcr_tracks *tracks_dev, uint64_t *out_dev,
                  int32_t n_out, void *stream);
/* survivor records for the all-gather of final tracks (compute.py:233-242 concatenation):
 * packed[r] = { lon[ns], lat[ns], v[ns], m[ns], vmax[ns], envw[ns][4] } of track idx[r],
 * r < min(*count_dev, cap); rows are row_stride doubles apart (0 = 9 * ns; larger leaves room for the
 * caller's own columns, e.g. candidate index / month / basin). */
int tcr_pack_tracks_dev(tcr_ctx *ctx, const tcr_tracks *src_dev, const int32_t *idx_dev,
                        const int64_t *count_dev, int64_t cap, double *packed_dev, int64_t row_stride, void *stream);
/* the same from fp32 rows; the packed records are fp64 (the 9-tuple is float64 like the reference's) */
int tcr_pack_tracks_f32_dev(tcr_ctx *ctx, const tcr_tracks_f32 *src_dev, const int32_t *idx_dev,
                            const int64_t *count_dev, int64_t cap, double *packed_dev, int64_t row_stride, void *stream);
/* tcr_pack_tracks_dev with the three columns run_tracks keeps next to a track's rows (compute.py:206-208) appended to
 * every record — packed[r][9*ns + 0..2] = global candidate index (cand0 + cand_idx[j], cand_idx NULL: cand0 + j), month
 * (slot[j] + 1), genesis-basin index (basin_idx[j]) of dense-batch row j = idx[r]; row_stride >= 9*ns + 3.  `f32` != 0:
 * src_dev is a tcr_tracks_f32. */
int tcr_pack_tracks_meta_dev(tcr_ctx *ctx, const tcr_tracks *src_dev, int32_t f32, const int32_t *idx_dev,
                             const int64_t *count_dev, int64_t cap, double *packed_dev, int64_t row_stride,
                             const int32_t *cand_idx_dev, const int32_t *slot_dev, const int32_t *basin_idx_dev,
                             int64_t cand0, void *stream);
/* replaces: `n_seeds[basin_idx, month - 1] += 1` (compute.py:165-167) for a finished round of candidates: out_dev[7][12]
 * (int64, SET) = candidates [cand0, cand0 + cand_dev->n) that count toward n_seeds (seed_flags bit 0) per (genesis basin,
 * month); with cutoff_dev (device scalar, a candidate index held as a double as the survivor records hold it) only the
 * candidates with global index <= *cutoff_dev — the candidate that completed the quota.
 * One stream per context: the reduction goes through a scratch block (partial counts + a ticket word) the CONTEXT owns, like
 * every workspace of the integrator, so two calls of the same context — this one or a tcr_round_dev with seed_hist — must be
 * enqueued on the same stream (or ordered by events); calls of different contexts are independent. */
int tcr_seed_hist_dev(tcr_ctx *ctx, const tcr_seeds *cand_dev, int64_t cand0, const double *cutoff_dev,
                      int64_t *out_dev, void *stream);

/* ---- one round of the accept loop in one call ------------------------------------------------------------------ */
/* replaces: one pass of the body of run_tracks' `while nt < n_tracks` loop (compute.py:134-209) over a block of
 * candidates — and, one level up, the fan-out of run_downscaling (compute.py:223-242), which hands run_tracks calls to
 * dask workers: here a round is ONE library call that enqueues
 *     tcr_seed_dev -> tcr_compact_dev (seeds that passed) -> tcr_cell_order_dev -> tcr_gather_seeds_dev ->
 *     tcr_integrate[_f32]_dev -> tcr_stats_dev -> tcr_compact_dev (accepted tracks) -> tcr_pack_tracks_meta_dev ->
 *     tcr_seed_hist_dev
 * on `stream`, with nothing returning to the host in between; every stage is optional through a NULL buffer.  The results
 * are exactly those of the separate calls, bit for bit (the same arithmetic; the round fuses a few of the small launches:
 * the locality order's cell keys come out of the compaction, the statistics out of the last post-processing kernel).  All
 * pointers are device memory and the caller owns them; they must stay valid until the stream has run the round. */
typedef struct {
    int64_t n_cand;             /* candidates of the round: [cand0, cand0 + n_cand) */
    int64_t n_storms;           /* capacity of the dense batch: the first n_storms passing seeds are integrated */
    tcr_seeds cand;             /* [n_cand] candidate arrays (cand.n is ignored; phases may be NULL, see tcr_seed_dev) */
    tcr_seeds storms;           /* [n_storms] the dense batch (storms.n is ignored) */
    int32_t *cand_idx;          /* [n_storms] position in the candidate block of every dense-batch storm */
    int64_t *n_passed;          /* [1] seeds that passed (may exceed n_storms) */
    double cell_deg;            /* > 0: dense batch in locality order (tcr_cell_order_dev); 0: candidate order */
    int32_t exact_count;        /* 1: integrate min(n_storms, *n_passed) storms (tcr_storms.n_dev); 0: the caller sized the
                                   round so that n_storms seeds pass (short rounds show in stats[6]) */
    int32_t f32;                /* 1: `tracks` is a tcr_tracks_f32 (tcr_integrate_f32_dev) */
    tcr_tracks tracks;          /* [n_storms] outputs */
    uint64_t *stats;            /* [TCR_N_STATS] added to (tcr_stats_dev), or NULL */
    int32_t *acc_idx;           /* [n_storms] dense-batch rows of the accepted tracks, or NULL (then no packing) */
    int64_t *n_accepted;        /* [1] */
    double *packed;             /* [pack_cap][pack_stride] survivor records (tcr_pack_tracks_dev; with the meta columns of
                                   tcr_pack_tracks_meta_dev when pack_stride >= 9 * n_steps + 3), or NULL */
    int64_t pack_cap, pack_stride;
    int64_t *seed_hist;         /* [7][12] the round's n_seeds contribution (tcr_seed_hist_dev, no cutoff), or NULL */
    int64_t n_expected;         /* 0, or how many seeds the caller expects to pass (<= n_storms): the integrator's launch is
                                   shaped for that many storms instead of the batch's capacity; never changes a result */
} tcr_round;
/* use_graph != 0: the round is captured into a hipGraph the first time a (ctx, descriptor) pair is seen and replayed from
 * then on — one graph launch instead of ~20 kernel launches: half the host time of a round (it is not what bounds small
 * rounds: DESIGN.md section 9, round 4).  The graph
 * is keyed by the descriptor's bytes; it is dropped whenever the context allocates or its parameters change.  seed / year /
 * cand0 reach the replayed kernels through a device-side key that a one-thread launch refreshes in front of the graph.
 * The TCR_* scheduling knobs are read when the graph is captured.  Timing events (tcr_timing_enable) are not recorded by
 * replayed rounds.  A context is used from one stream at a time, as for every other entry point.
 * Capture is a process-wide affair in HIP: while a round is being captured (its first use), a legacy-default-stream
 * operation on ANY thread of the process — a synchronous hipMemcpy, a torch op on the default stream — fails there ("would
 * make the legacy stream depend on a capturing blocking stream") and invalidates the capture here; the descriptor then keeps
 * the direct form and no error is returned for it.  The library's own synchronous copies (field staging, host entry
 * points) go through the context's stream for that reason (tools/capture_race_probe.py: 3 700 captures next to threads
 * that stage fields, allocate and grow workspaces, no error); a caller that captures keeps its other threads off the
 * default stream.  The replay saves ~40 us of host time per round and no GPU time. */
int tcr_round_dev(tcr_ctx *ctx, const tcr_round *round, uint64_t experiment_seed, int32_t year, int64_t cand0,
                  int32_t use_graph, void *stream);
/* Stage trace of directly enqueued rounds (measurement aid; replayed rounds record nothing): with it enabled tcr_round_dev
 * records a HIP event behind every stage, and tcr_stage_trace_sum returns, per stage, the summed time from the previous
 * event of the stream to the stage's own — i.e. how long the stream took to get through that stage, waiting included —
 * over the *n_rounds rounds since the trace was enabled (which also resets it). */
enum { TCR_STAGE_START = 0, TCR_STAGE_SEED, TCR_STAGE_SELECT, TCR_STAGE_ORDER, TCR_STAGE_GATHER, TCR_STAGE_FOURIER,
       TCR_STAGE_INTEGRATE, TCR_STAGE_SCREEN, TCR_STAGE_SELECT_TC, TCR_STAGE_DENSE, TCR_STAGE_EMIT, TCR_STAGE_FLAGS,
       TCR_STAGE_STATS, TCR_STAGE_PACK, TCR_N_STAGES };
int tcr_stage_trace_enable(tcr_ctx *ctx, int on);
int tcr_stage_trace_sum(tcr_ctx *ctx, double ms[TCR_N_STAGES], int64_t *n_rounds);
/* graphs this context holds / replays since it was created (test and measurement aid) */
int tcr_round_graph_stats(tcr_ctx *ctx, int64_t *n_graphs, int64_t *n_replays);

/* ---- preprocessing next to the path ----------------------- */
/* replaces: calc_wnd_stat (track/env_wind.py:180-228) for one month: wnd[c] = ua250, va250,
 * ua850, va850 as [n_samples][n_points] planes (points = the flattened lat x lon grid); day_start
 * (NULL: samples are days) holds n_days + 1 sample offsets of the calendar days of a sub-daily
 * record (the reference's groupby("time.day").mean).  out = [14][n_points]: 4 means, then the lower
 * triangle of the covariance row by row, variances with ddof 0 and covariances with ddof 1 exactly as
 * the reference's .var / xr.cov give them.  _dev: device pointers, asynchronous on `stream`. */
int tcr_wind_stats_dev(tcr_ctx *ctx, int64_t n_samples, int64_t n_points, const double *const wnd[4],
                       const int32_t *day_start, int32_t n_days, double *out, void *stream);
int tcr_wind_stats_host(tcr_ctx *ctx, int64_t n_samples, int64_t n_points, const double *const wnd[4],
                        const int32_t *day_start, int32_t n_days, double *out);
/* The same for float32 planes — the dtype ERA5 u / v files hold and xarray keeps through .mean / .var / xr.cov:
 * sums over time in float32 in time order, divisions through fp64 rounded back to float32, covariances
 * (float32 sum / int64 count) in fp64, every statistic stored as fp64.  Both variants skip NaN samples as
 * xarray's skipna does (per pair for the covariances). */
int tcr_wind_stats_f32_dev(tcr_ctx *ctx, int64_t n_samples, int64_t n_points, const float *const wnd[4],
                           const int32_t *day_start, int32_t n_days, double *out, void *stream);
int tcr_wind_stats_f32_host(tcr_ctx *ctx, int64_t n_samples, int64_t n_points, const float *const wnd[4],
                            const int32_t *day_start, int32_t n_days, double *out);

/* ---- thermodynamic preprocessing ---------------------------- */
/* replaces: np.load(thermo/entropy_table.npz) in CAPE_PI_vectorized (thermo/thermo.py:272-277):
 * T[np][ns] over ascending pressure (Pa) and entropy (J/kg/K) axes. */
int tcr_entropy_table_upload(tcr_ctx *ctx, int32_t np, int32_t ns, const double *p, const double *s, const double *T);
/* replaces: thermo.CAPE_PI_vectorized(sst, p_surf, p_env, T_env, r_env) (thermo/thermo.py:266-412;
 * select_thermo = 1, select_interp = 2) for n_points columns: p_env[n_lev] in Pa from the lowest level up,
 * T_env / r_env as [n_lev][n_points] planes, ck_over_cd = namelist.Ck / namelist.Cd; pi[n_points] in m/s. */
int tcr_potential_intensity_host(tcr_ctx *ctx, int64_t n_points, int32_t n_lev, const double *p_env,
                                 const double *sst, const double *psl, const double *T_env, const double *r_env,
                                 double ck_over_cd, double *pi);
int tcr_potential_intensity_dev(tcr_ctx *ctx, int64_t n_points, int32_t n_lev, const double *p_env,
                                const double *sst, const double *psl, const double *T_env, const double *r_env,
                                double ck_over_cd, double *pi, void *stream);
/* replaces: thermo.sat_deficit (thermo/thermo.py:92-104, unclipped) and thermo.conv_q_to_rh (:41-46) at the
 * mid level p_mid (Pa), as thermo/calc_thermo.py:66-74 calls them. */
int tcr_chi_rh_host(tcr_ctx *ctx, int64_t n_points, const double *sst, const double *psl, const double *T_mid,
                    const double *q_mid, double p_mid, double *chi, double *rh_mid);

/* ---- gen_track(clon, clat, v, m=None) ---------------------------------------- */
/* replaces: Coupled_FAST._init_m(y, dvdt) (intensity/coupled_fast.py:153-173), which gen_track calls with dvdt = 0
 * when it is given no m (coupled_fast.py:258-261): the inner-core moisture that makes dv/dt equal `dvdt` at t = 0,
 * with the potential intensity taken as the maximum over the point and the four points 0.25 degrees diagonally off
 * it.  m_out[i] = storms->m0[i] where that is a number (or storms->m0 is not NULL and not NaN), else _init_m's value
 * (storms->m0 may be NULL: every storm is initialised).  run_tracks always passes m (compute.py:173-176), so the
 * integrate entry points require m0; a caller that wants the reference's m=None behaviour calls this first and hands
 * m_out to tcr_integrate_* as m0.  Uses lon0, lat0, v0, h_bl, slot and phases (the env winds at t = 0). */
int tcr_init_m_dev(tcr_ctx *ctx, const tcr_storms *storms_dev, double dvdt, double *m_out_dev, void *stream);
int tcr_init_m_host(tcr_ctx *ctx, const tcr_storms *storms_host, double dvdt, double *m_out_host);

/* ---- single-point probes (parity tests of the seam's leaf methods) -------- */
/* (tests) the arithmetic helpers of the integrator on their own (csrc/tcr_device.h, "Arithmetic policy"): out[i] = fn(a[i][, b[i]]),
 * fn 0: a / b without range scaling (qdiv_nz), 1: sqrt (qsqrt), 2: sqrt of a positive argument (qsqrt_pos), 3: a ** (-1/5)
 * (inv_fifth_root: err ** -0.2 of scipy/integrate/_ivp/rk.py:160), 4: a ** -0.4 (strat_pow: t_strat ** -0.4,
 * intensity/coupled_fast.py:91), 5: cos(a) for a in [-pi / 2, pi / 2] (cos_lat: np.cos(np.deg2rad(lat)), track/bam_track.py:139).
 * fn 6-12: the float instantiations the fp32 variant runs — 6: qdiv_nz<float> (a / b), 7: qsqrt<float>, 8: qsqrt_pos<float>,
 * 9: inv_fifth_root<float> (pow(a, -0.2f)), 10: strat_pow<float> (pow(a, -0.4f)), 11: cos_lat<float>, 12: exp(-a) in float (the
 * ocean feedback's exponential, coupled_fast.py:94); operands are rounded to float on the device, results widened to double.
 * Host arrays; b may be NULL except for fn 0 and 6. */
int tcr_probe_math_host(tcr_ctx *ctx, int32_t fn, int64_t n, const double *a, const double *b, double *out);
/* replaces: Coupled_FAST.dydt (coupled_fast.py:196-207), ._env_winds
 * (bam_track.py:116-128) and ._calc_alpha (coupled_fast.py:65-94) at n points
 * of one slot with one forcing table Fs[4][n_steps] (host buffers). */
int tcr_probe_rhs_host(tcr_ctx *ctx, int slot, double h_bl, const double *Fs, int64_t n,
                       const double *t, const double *lon, const double *lat,
                       const double *v, const double *m,
                       double *dydt /*[n][4]*/, double *envw /*[n][4]*/, double *alpha /*[n]*/);
/* (tests) the same evaluation in the arithmetic of the fp32 variant (tcr_integrate_f32_*): the float fields, knots and constants
 * that variant stages, Fs and h_bl rounded to float on the host, lon / lat / v / m rounded to float on the device, t kept in double;
 * results widened to double.  aux (may be NULL) is [n][24]: the lookups of that very evaluation — the 14 wind lookups (4 means,
 * 10 packed covariances), vpot, chi, mld, strat, land, bathymetry, then the PI in use (0 over land), chi, the decision bits
 * (bit0 `land == 1`, bit1 PI != 0, bit2 |land - 1| <= 1e-12) and one pad. */
int tcr_probe_rhs_f32_host(tcr_ctx *ctx, int slot, double h_bl, const double *Fs, int64_t n,
                           const double *t, const double *lon, const double *lat,
                           const double *v, const double *m,
                           double *dydt /*[n][4]*/, double *envw /*[n][4]*/, double *alpha /*[n]*/, double *aux /*[n][24] or NULL*/);
/* Test instrument of Coupled_FAST._get_over_land (coupled_fast.py:35-38): tcr_integrate_host plus, per storm,
 * one byte per evaluation of dydt in call order — bit0 = `f_land.ev(lon, lat) == 1`, bit1 = the interpolated
 * PI is non-zero, bit2 = the land value is within 1e-12 of 1; 0xff = not evaluated.  dec is [n][cap] host
 * memory.  That decision is taken by rounding in the interior of land, so parity tests compare tracks up
 * to the first evaluation where it lands differently (oracle/parity.py).  Results equal tcr_integrate_host's. */
int tcr_integrate_probe_host(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks *out, uint8_t *dec, int32_t cap);
/* Test instrument of the RK45 step (tests/test_rk_steps.py): tcr_integrate_host / tcr_integrate_f32_host plus the batch's
 * accepted-step records as the integrator left them, copied before the dense-output kernel rewrites them.  steps is host memory
 * [n][max_rk_steps][REC] doubles, REC = 36 (fp64) or 20 (fp32), and steps_doubles must be exactly that count (max_rk_steps = 64
 * when tcr_params.max_rk_steps <= 0).  A record is doubles t_old, h, t_new, one pad; then in the run's type (double, or float
 * packed two to a double) y_old[4] and the seven stage derivatives K[7][4].  Storm i has min(n_accept[i], max_rk_steps) records;
 * gated storms have none; what lies behind a storm's last record is stale memory.  Results equal the plain entry point's.
 * While a call is in progress the _dev entry points and tcr_round_dev on the same context fail. */
int tcr_integrate_steps_host(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks *out, double *steps, int64_t steps_doubles);
int tcr_integrate_steps_f32_host(tcr_ctx *ctx, const tcr_storms *in, const tcr_tracks_f32 *out, double *steps, int64_t steps_doubles);
/* replaces: gen_f (bam_track.py:23-31): Fs[n][4][n_steps] from phases[n][4][n_series] */
int tcr_fourier_table_host(tcr_ctx *ctx, int64_t n, const double *phases, double *Fs);

/* ---- measurement ----------------------------------------------------------- */
/* HIP-event durations (ms) of the kernels of the last tcr_integrate_dev/_host
 * call on this context: [0] fourier table, [1] integrate, [2] post/unpack.
 * Enabled by tcr_timing_enable(ctx, 1) (which also resets the record); reading
 * waits for the recorded events.  Events are recorded on the launch stream. */
int tcr_timing_enable(tcr_ctx *ctx, int on);
int tcr_timing_last(tcr_ctx *ctx, double ms[3]);
/* sums over every timed call since tcr_timing_enable(ctx, 1); *n_calls = how many */
int tcr_timing_sum(tcr_ctx *ctx, double ms[3], int64_t *n_calls);
/* Occupancy accounting of the last tcr_integrate_* call (synchronises the device first is the
 * caller's job): k_integrate runs as a chain of passes (tail compaction); for each pass p
 * out[6p..6p+5] = { queue requests, storms parked for pass p+1, wave cycles, live-lane cycles,
 * wave wall-clock ticks at 100 MHz, wave shader-clock ticks }.  One cycle = one RK45 step attempt (six evaluations of
 * the reference's ode_rhs, intensity/coupled_fast.py:150-209) of up to 64 storms; live-lane
 * cycles / (64 x wave cycles) is the lane utilisation.  Returns the number of passes. */
int tcr_integrate_pass_stats(tcr_ctx *ctx, int64_t *out, int max_passes);
int tcr_sync(tcr_ctx *ctx, void *stream);

/* ---- multi-GPU: the exchange of final tracks, RCCL over xGMI ---------------------------------------------------- */
/* replaces: the fan-out / collection of run_downscaling (util/compute.py:223-242) — the reference hands run_tracks calls to
 * dask worker processes and gets their 9-tuples pickled back.  Here one process owns one GPU and one context; every rank
 * integrates its share (a block of each round's candidate indices, or whole years) and the survivor records are exchanged with
 * ONE fixed-shape ncclAllGather per round / per run, device to device.  RCCL is loaded at run time (dlopen of librccl.so.1 —
 * the copy the process already holds, e.g. PyTorch's, when there is one): a single-GPU user never needs it.
 *   rank 0: tcr_comm_unique_id(id) -> the 128 bytes travel to the other ranks by any host channel (a file, MPI, a TCP store)
 *   all   : tcr_comm_create(ctx, id, rank, world, &comm)       collective: every rank of the job calls it
 * A communicator borrows its context (error text, device, default stream): destroy it before the context.
 * Calls on one communicator are collective and must be issued in the same order on every rank; they are asynchronous on
 * `stream` (NULL: the context's).  Ragged contributions travel padded to a common row count (`cap`), each rank's real count
 * next to them (tcr_allgather_counts_dev); tcr_concat_rows_dev packs the received blocks in rank order — which is candidate
 * order when ranks own contiguous candidate blocks in rank order (the order the reference's sequential loop meets them). */
#define TCR_COMM_ID_BYTES 128
typedef struct tcr_comm tcr_comm;
int tcr_comm_unique_id(uint8_t id[TCR_COMM_ID_BYTES]);     /* errors: tcr_last_error(NULL) */
int tcr_comm_create(tcr_ctx *ctx, const uint8_t id[TCR_COMM_ID_BYTES], int32_t rank, int32_t world, tcr_comm **out);
int tcr_comm_destroy(tcr_comm *comm);
int tcr_comm_rank(const tcr_comm *comm);
int tcr_comm_world(const tcr_comm *comm);
/* recv_dev[world][bytes] <- every rank's send_dev[bytes] (the same size on every rank) */
int tcr_allgather_dev(tcr_comm *comm, const void *send_dev, void *recv_dev, int64_t bytes, void *stream);
/* gathered_dev[world][n_rows][row_stride] <- every rank's rows_dev[n_rows][row_stride] (survivor records: row_stride =
 * 9 * n_steps (+ 3 meta columns), tcr_pack_tracks[_meta]_dev) */
int tcr_allgather_rows_dev(tcr_comm *comm, const double *rows_dev, int64_t n_rows, int64_t row_stride, double *gathered_dev, void *stream);
/* counts_dev[world] <- every rank's *count_dev */
int tcr_allgather_counts_dev(tcr_comm *comm, const int64_t *count_dev, int64_t *counts_dev, void *stream);
/* buf_dev[n] <- sum over ranks, in place (n_seeds[7][12], compute.py:167; round control) */
int tcr_allreduce_sum_i64_dev(tcr_comm *comm, int64_t *buf_dev, int64_t n, void *stream);
/* out_dev[sum_r min(counts[r], cap)][row_stride] <- the first min(counts[r], cap) rows of every rank's block of
 * gathered_dev[n_blocks][cap][row_stride] (n_blocks = world), in rank order; at most out_cap rows are written;
 * *n_out_dev (optional) = rows written.  Local to the calling rank (no communication). */
int tcr_concat_rows_dev(tcr_ctx *ctx, int32_t n_blocks, const double *gathered_dev, const int64_t *counts_dev, int64_t cap, int64_t row_stride,
                        double *out_dev, int64_t out_cap, int64_t *n_out_dev, void *stream);

/* ---- site hazard: near-site intensity and exceedance counts ------------------------------------------------------- */
/* replaces: the analysis of notebooks/sample_analysis.ipynb on a track file, for n_site sites at once:
 *   max[site][storm]          = nanmax of vmax over the live samples (lon, lat not NaN) within radius_km of the site, by the
 *                               notebook's haversine (r_earth = 6378 km; NaN when there are none)
 *   counts[site][g][b] (int32) = #storms s in [group_off[g], group_off[g + 1]) with max[site][s] >= thresholds[b]
 * lon / lat / vmax are the track file's lon_trks / lat_trks / vmax_trks, [n_trk][row_stride] with n_t samples used per row; sites
 * and tracks may use either longitude convention.  0 < radius_km <= 5000, 1 <= n_bin <= 64, thresholds finite and strictly
 * ascending, group_off non-decreasing from 0 to n_trk.  Results are bit-identical from run to run and do not depend on the
 * order of the sites; storms and sites far apart are skipped in blocks, so sites given in a spatially coherent order (runs of 64
 * neighbours) run fastest.  site_max (optional, NULL: not written) is [n_site][n_trk].
 * _dev: lon / lat / vmax, site_lon / site_lat, counts and site_max are device memory, asynchronous on `stream`;
 * group_off and thresholds are host memory in both entry points.  Workspaces belong to the context (grown on demand): calls on
 * one context must be ordered (one stream, or the previous call finished). */
typedef struct {
    int64_t n_trk, n_t, row_stride;
    const double *lon, *lat, *vmax;
    int32_t n_group;
    const int64_t *group_off;              /* host, [n_group + 1] */
} tcr_hazard_tracks;
int tcr_hazard_dev(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, int64_t n_site, const double *site_lon, const double *site_lat,
                   double radius_km, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max, void *stream);
int tcr_hazard_host(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, int64_t n_site, const double *site_lon, const double *site_lat,
                    double radius_km, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max);
/* (site, sample) distance tests the last tcr_hazard_* call of this context evaluated after culling; waits for that call */
int tcr_hazard_pairs(tcr_ctx *ctx, int64_t *pairs);

/* ---- landfall: sea -> land steps of the model's land decision ---------------------------------------------------- */
/* replaces: nothing in the reference's code (its README's landfall return periods); the land decision is the one the model
 * switches its physics on, f_land.ev(lon, lat) == 1 on the bilinear interpolant of intensity/data/land.nc, taken on the nodes:
 *   land node       land >= 1 (NaN: water)
 *   sample's cell   by comparisons only: i = the last lon node <= x (0 below the grid: clamped as FITPACK does); node i + 1 has
 *                   a nonzero weight iff it exists and lon_i < x; the same for lat.  A grid is periodic when
 *                   lon[nlon-1] - lon[0] + (lon[1] - lon[0]) == 360 exactly: x is reduced first, t = fmod(x - lon0, 360),
 *                   t += 360 when t < 0, x = lon0 + t (lon0 when that rounds to lon0 + 360), and the last cell wraps to node 0.
 *   over land       every node with a nonzero bilinear weight is a land node (no arithmetic: the `== 1` flicker does not enter)
 *   event           a live sample k (lon, lat not NaN) over land whose previous live sample p is not; per event: k, lon[k],
 *                   lat[k], v_landfall = vmax[p], v_inland = vmax[k] (NaN kept).  A storm that starts over land has no event there.
 * Hourly samples can step over a land strip narrower than an hour's motion: such a crossing is not an event.
 * tcr_land_upload: nlon, nlat >= 2, lon / lat finite and strictly ascending, land [nlat][nlon] (host memory); replaces the
 * context's grid (no tcr_landfall_* call of the context may be in flight).  tcr_land_info: the uploaded grid's sizes and periodic flag.
 * tcr_landfall_*: the tracks' group fields are ignored.  n_landfall [n_trk] (int32) counts every event; the first
 * min(n_landfall, max_events) go to ev_k (int32), ev_lon, ev_lat, ev_v, ev_v_inland [n_trk][max_events] in order, the rest of a
 * row is ev_k = -1 and NaN.  max_events >= 0 (0: counts only; the event planes may be NULL).  flags (optional, NULL: not
 * written) [n_trk][n_t] uint8: 0 water, 1 land, 2 not live.  Results are copies of inputs and integers: bit-identical from run to
 * run.  _dev: tracks and outputs are device memory, asynchronous on `stream`. */
typedef struct {
    int64_t nlon, nlat;
    const double *lon, *lat;               /* host, [nlon], [nlat] */
    const double *land;                    /* host, [nlat][nlon] */
} tcr_land_grid;
int tcr_land_upload(tcr_ctx *ctx, const tcr_land_grid *grid);
int tcr_land_info(tcr_ctx *ctx, int64_t *nlon, int64_t *nlat, int32_t *periodic);
int tcr_landfall_dev(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, int32_t max_events, int32_t *n_landfall, int32_t *ev_k,
                     double *ev_lon, double *ev_lat, double *ev_v, double *ev_v_inland, uint8_t *flags, void *stream);
int tcr_landfall_host(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, int32_t max_events, int32_t *n_landfall, int32_t *ev_k,
                      double *ev_lon, double *ev_lat, double *ev_v, double *ev_v_inland, uint8_t *flags);

/* ---- track climatology: track, exceedance, genesis and LMI density, PDI -------------------------------------------- */
/* replaces: nothing in the reference's code (its README's track density, genesis locations, LMI distributions and
 * power dissipation, which users compute in NumPy over the track planes).  A sample is live when lon and lat are not NaN.
 *   grid            tcr_clim_grid: dlon, dlat > 0, nlon, nlat >= 1, nlon * dlon <= 360, nlon * nlat < 2^31, all finite.
 *                   Longitude: t = fmod(x - lon0, 360), t += 360 when t < 0, t = 0 when that rounds to 360, i = floor(t / dlon);
 *                   a global grid (nlon * dlon == 360 exactly) clamps i to nlon - 1, any other grid leaves i >= nlon outside.
 *                   Latitude: j = floor((y - lat0) / dlat), inside iff 0 <= j < nlat.  The cell is this arithmetic, so tracks
 *                   in either longitude convention (or lon > 360) land in the same cell.  Cell (j, i) is j * nlon + i.
 *   q(v)            (int64) rint(((v * v) * v) * 1024.0) in fp64 without contraction for 0 <= v <= 400, else 0; the physical
 *                   PDI is q / 1024 * dt (m^3 s^-2, dt the sample spacing).  Integer sums: bit-identical whatever the launch
 *                   shape and the storm order.
 * Maps, [n_group][nlat][nlon], overwritten by every call, of the storms s with group[s] in [0, n_group):
 *   track (int32)   storms with at least one live sample in the cell (once per cell, however often the storm comes back)
 *   exceed (int32)  [n_group][n_bin][nlat][nlon]: storms whose NaN-skipping max of vmax over their live samples in the cell
 *                   is >= thresholds[b] (NULL when n_bin == 0)
 *   genesis (int32) storms whose first live sample is in the cell
 *   lmi (int32)     storms whose lifetime-maximum sample is in the cell: the first sample attaining the NaN-skipping max of
 *                   vmax over the storm's live samples
 *   pdi (int64)     sum of q(vmax) over the live samples in the cell
 * Per storm, [n_trk]: genesis_k (int32, the first live sample, -1 when none), lmi_v (the lifetime maximum, NaN when no live
 * sample has a non-NaN vmax), lmi_k (int32, its sample, -1 when none), pdi_storm (int64, q summed over the live samples).
 * Samples outside the grid add nothing to the maps but count in the per-storm outputs; a storm whose group is out of range adds
 * nothing to the maps.  Samples are points: a storm can step over a cell smaller than an hour's motion without a sample in it.
 * Arguments: n_trk >= 0, 1 <= n_t, row_stride >= n_t, n_trk * n_t <= 2^27 (the int64 sums cannot overflow), n_group >= 1,
 * 0 <= n_bin <= 64, thresholds (host) finite and strictly ascending.  The tracks' group fields are ignored.  n_trk == 0 zeroes
 * the maps and writes nothing else.  _dev: tracks, group and outputs are device memory, asynchronous on `stream`; tracks longer
 * than 512 samples sort in a workspace of the context (grown on demand): calls on one context must be ordered. */
typedef struct {
    double lon0, dlon, lat0, dlat;
    int64_t nlon, nlat;
} tcr_clim_grid;
typedef struct {
    int32_t *track, *exceed, *genesis, *lmi;   /* [n_group][nlat][nlon]; exceed [n_group][n_bin][nlat][nlon] */
    int64_t *pdi;                              /* [n_group][nlat][nlon] */
    int32_t *genesis_k;                        /* [n_trk] */
    double *lmi_v;                             /* [n_trk] */
    int32_t *lmi_k;                            /* [n_trk] */
    int64_t *pdi_storm;                        /* [n_trk] */
} tcr_clim_out;
int tcr_climatology_dev(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, const int32_t *group, int32_t n_group,
                        const tcr_clim_grid *grid, int32_t n_bin, const double *thresholds, const tcr_clim_out *out, void *stream);
int tcr_climatology_host(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, const int32_t *group, int32_t n_group,
                         const tcr_clim_grid *grid, int32_t n_bin, const double *thresholds, const tcr_clim_out *out);

/* ---- wind footprint: peak wind at sites from a radial profile around the centre ---------------------------------- */
/* replaces: nothing in the reference's code; extends its axi_to_max_wind (wind/tc_wind.py) from one number per sample to the
 * wind each sample produces at each site.  R = 6378.1 km (util/constants.py earth_R), Omega = 7.292e-5 s^-1, SI units.
 *   track           a storm's leading run of n samples where lon, lat, v, u250, v250, u850, v850 are all finite (later samples
 *                   are ignored).  A track of one sample has no translation speed and contributes nothing.
 *   per sample k    (ut, vt) of calc_translational_speed (util/sphere.py, linear extrapolation at both ends, dt = dt_s) in the
 *                   operation order of the pipeline's vmax_trks; G, Ui, Vi, |U|, fac = min(1, 0.5 v / |U|) as tc_wind.py:7-16,
 *                   A = fac (Ui, Vi).  rm (km) = rmax_km[k] when the plane is given, else rmax_const_km when > 0, else
 *                   Willoughby, Darling & Rahn (2006, eq. 7a) 46.4 exp(-0.0155 v + 0.0169 |lat|).  f = 2 Omega |sin lat|,
 *                   Mm = rm v + f rm^2 / 2.
 *   sub-steps       substeps = n >= 1: between track samples k and k + 1, sub-samples at tau = j / n, j = 1 .. n - 1, with lat, v,
 *                   rm and both components of A linear in tau (y_k + tau (y_k+1 - y_k)), lon the same with its difference reduced
 *                   to [-180, 180); f and Mm from the interpolated values.
 *   per (site, s)   r = haversine distance with R; the sample is included iff r <= r_out_km.  c = ck_cd, x = r / rm,
 *                   ratio = [2 x^2 / (2 - c + c x^2)]^(1 / (2 - c)) (Emanuel & Rotunno 2011, eq. 36),
 *                   V = max(0, (Mm ratio - f r^2 / 2) / r), V = 0 at r = 0; V(rm) = v.  d = (e, n) / |(e, n)| with
 *                   e = cos phi_s sin(lam_s - lam_c), n = cos phi_c sin phi_s - sin phi_c cos phi_s cos(lam_s - lam_c);
 *                   t = h (-d_n, d_e), h = +1 for lat >= 0 and -1 otherwise; wind = |V t + (V / v) A|, 0 when v <= 0.
 *                   At r = rm its maximum over azimuth is v + fac |U|, axi_to_max_wind's vmax.
 *   site_max        [n_site][n_trk] (optional, NULL: not written): max of the wind over the included samples and sub-samples of
 *                   the storm, NaN when none is included.
 *   counts          [n_site][n_group][n_bin] (int32): storms s in [group_off[g], group_off[g + 1]) with site_max >= thresholds[b].
 * Arguments: dt_s > 0, 0 < ck_cd < 2, 0 < r_out_km <= 2000, 1 <= substeps <= 64, rmax_const_km >= 0 (0 when the plane is given),
 * 1 <= n_bin <= 64, thresholds finite and strictly ascending, group_off non-decreasing from 0 to n_trk; rm > 0 and finite at
 * every sample of a track (tcr_windfield_host checks the plane; tcr_windfield_dev cannot, and drops a storm with a bad rm:
 * NaN at every site, counted nowhere).  Results are a max of per-pair values and integer counts: bit-identical from run to run,
 * whatever the launch shape, the site order or the storm order.  Sites in a spatially coherent order (runs of 64 neighbours)
 * run fastest.  _dev: planes, sites, counts and site_max are device memory, asynchronous on `stream`; group_off and thresholds
 * are host memory in both entry points.  Workspaces belong to the context (grown on demand): calls on one context must be
 * ordered (one stream, or the previous call finished). */
typedef struct {
    int64_t n_trk, n_t, row_stride;
    const double *lon, *lat, *v, *u250, *v250, *u850, *v850;
    const double *rmax_km;                 /* [n_trk][row_stride] in km, or NULL */
    int32_t n_group;
    const int64_t *group_off;              /* host, [n_group + 1] */
} tcr_wind_tracks;
typedef struct {
    double dt_s, ck_cd, r_out_km, rmax_const_km;
    int32_t substeps;
} tcr_wind_params;
int tcr_windfield_dev(tcr_ctx *ctx, const tcr_wind_tracks *tracks, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                      const double *site_lat, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max, void *stream);
int tcr_windfield_host(tcr_ctx *ctx, const tcr_wind_tracks *tracks, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                       const double *site_lat, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_max);
/* (site, sample or sub-sample) pairs the last tcr_windfield_* call of this context evaluated after culling; waits for that call */
int tcr_windfield_pairs(tcr_ctx *ctx, int64_t *pairs);

/* ---- portfolio loss: event losses, year losses and loss-cost map of exposed values under the wind footprint -------- */
/* replaces: nothing in the reference's code; puts a damage function on the wind footprint above and sums it over the sites inside
 * the scan, so that the site_max[n_site][n_trk] matrix never exists.  The damage function is Emanuel (2011, "Global warming
 * effects on U.S. hurricane damage", eq. 1), with the constants CLIMADA uses as its defaults (v_thresh = 25.7, v_half = 74.7 m/s).
 *   m               site_max[i][s] of tcr_windfield_* for the same tracks, parameters and sites (NaN: no sample within r_out_km)
 *   loss[i][s]      site_value[i] D,  D = x^3 / (1 + x^3),  x = max(m - v_thresh, 0) / (v_half_i - v_thresh);  0 when m is NaN.
 *                   D(v_thresh) = 0, D(v_half) = 1/2, D -> 1.  v_half_i = site_v_half[i], or v_half when site_v_half is NULL.
 *   event_loss      [n_trk]: sum over the sites of loss[i][s] (the event loss table)
 *   year_agg        [n_group]: sum of event_loss over the storms of the group;  year_max [n_group]: their maximum.  Both 0 for a
 *                   group without storms.
 *   site_loss       [n_site]: sum over all storms of loss[i][s] (divided by the years: a loss-cost map)
 *   counts          [n_site][n_group][n_bin] (int32): the footprint's exceedance counts, as tcr_windfield_* gives them
 * Arguments: those of tcr_windfield_* under the same rules (their messages begin with "tcr_windfield:"), and v_thresh finite and
 * >= 0, v_half finite and > v_thresh; site_value finite and >= 0 and site_v_half finite and > v_thresh at every site.
 * tcr_loss_host checks the two site arrays; tcr_loss_dev cannot, and a site with a bad value or a bad v_half contributes 0 to
 * every sum (its counts are still the footprint's).  No floating-point atomics: sites are summed per run of 64 consecutive sites
 * by a fixed butterfly and the runs in ascending order, so event_loss[s] is bit-identical from run to run and does not depend on
 * the other storms of the call or on their order; year_max likewise; year_agg depends on the storms of its group and their
 * order, site_loss on the storm order and the group offsets.  Workspace: (n_site / 64) x n_trk doubles and one double per
 * (site, chunk of storms), grown on demand; when it does not fit the call fails ("split the sites").  _dev: planes, sites,
 * site_value, site_v_half and all outputs are device memory, asynchronous on `stream`; group_off and thresholds are host memory
 * in both entry points.  The workspace is the context's third (next to the hazard's and the footprint's): calls of tcr_loss_* on
 * one context must be ordered, but one may be in flight next to a tcr_windfield_* or tcr_hazard_* call on another stream. */
typedef struct {
    double v_thresh, v_half;
} tcr_loss_params;
int tcr_loss_dev(tcr_ctx *ctx, const tcr_wind_tracks *tracks, const tcr_wind_params *wind, const tcr_loss_params *loss, int64_t n_site,
                 const double *site_lon, const double *site_lat, const double *site_value, const double *site_v_half, int32_t n_bin,
                 const double *thresholds, int32_t *counts, double *event_loss, double *year_agg, double *year_max, double *site_loss,
                 void *stream);
int tcr_loss_host(tcr_ctx *ctx, const tcr_wind_tracks *tracks, const tcr_wind_params *wind, const tcr_loss_params *loss, int64_t n_site,
                  const double *site_lon, const double *site_lat, const double *site_value, const double *site_v_half, int32_t n_bin,
                  const double *thresholds, int32_t *counts, double *event_loss, double *year_agg, double *year_max, double *site_loss);

/* ---- rainfall footprint: storm-total rain and peak rain rate at sites from a radial rain-rate profile ---------------- */
/* replaces: nothing in the reference's code; the freshwater half of the risk, on the three planes every track file has.  The rate
 * is R-CLIPER (Tuleya, DeMaria & Kuligowski 2007): a function of the distance from the centre and of vmax alone.  R = 6378.1 km
 * (util/constants.py earth_R), as in the wind footprint.
 *   track           a storm's leading run of n samples where lon, lat and vmax are all finite (later samples are ignored; the
 *                   wind footprint's rule, not the hazard's compaction: time weights need contiguous samples).  A track of
 *                   fewer than 2 samples has no records.
 *   records         substeps = m >= 1: the track samples, and between samples k and k + 1 sub-samples at tau = j / m,
 *                   j = 1 .. m - 1, with lat and vmax linear in tau (y_k + tau (y_k+1 - y_k)), lon the same with its difference
 *                   reduced to [-180, 180) (the short way round): n_rec = (n - 1) m + 1 records, in time order.  Record q
 *                   carries the trapezoid weight w_q = dt_s / (3600 m) hours, halved for q = 0 and q = n_rec - 1.
 *   rate (mm/h)     of a record at distance r (km):
 *                     V_kt = clamp(vmax 3600 / 1852, v_lo_kt, v_hi_kt),  U = 1 + (V_kt - 35) / 33
 *                     T0 = a[0] + b[0] U,  Tm = a[1] + b[1] U   (inches / day);   rm = a[2] + b[2] U,  re = a[3] + b[3] U   (km)
 *                     rate_in_day = T0 + (Tm - T0) r / rm  for r < rm,   Tm exp(-(r - rm) / re)  for r >= rm
 *                     rate = max(rate_in_day, 0) 25.4 / 24
 *                   Defaults (the callers': the library has none) are the TRMM fit, a = (-1.10, -1.60, 64.5, 150.0),
 *                   b = (3.96, 4.80, -13.0, -16.0), and the clamp v_lo_kt = 35, v_hi_kt = 155: a depression rains like a
 *                   minimal tropical storm, and with these coefficients rm(U) reaches zero at 165.7 kt (U = 64.5 / 13).
 *   per (site, q)   r = haversine distance with R; the record is included iff r <= r_out_km.
 *   site_value      [n_site][n_trk] (optional, NULL: not written), NaN when no record of the storm is included at the site;
 *                   stat = TCR_RAIN_TOTAL: the sum of w_q rate_q(r) over the included records, added in record order (mm);
 *                   stat = TCR_RAIN_PEAK_RATE: the max of rate_q(r) over the included records (mm/h).
 *   counts          [n_site][n_group][n_bin] (int32): storms s in [group_off[g], group_off[g + 1]) with site_value >= thresholds[b].
 * Arguments: dt_s finite and > 0, 0 < r_out_km <= 2000, 1 <= substeps <= 64, stat 0 or 1, 0 < v_lo_kt <= v_hi_kt finite, all
 * eight coefficients finite, and rm > 0, re > 0, Tm >= 0 at both clamp ends (all are linear in U, so also in between; T0 may be
 * negative: the rate is clamped at 0); n_trk >= 0, 1 <= n_t <= 2^20, row_stride >= n_t, 1 <= n_bin <= 64, thresholds finite and
 * strictly ascending, group_off non-decreasing from 0 to n_trk.  Every message begins with "tcr_rainfall:".
 * Not modelled: rain asymmetry from shear or topography, and decay after landfall.
 * A site's sum of a storm is one accumulator over exactly the included records in record order, whatever else the call holds
 * (skipped blocks of far storms contain no included record), and the max and the integer counts do not depend on order: results
 * are bit-identical from run to run, whatever the launch shape, the site order or the storm order.  Sites in a spatially coherent
 * order (runs of 64 neighbours) run fastest.  _dev: planes, sites, counts and site_value are device memory, asynchronous on
 * `stream`; group_off and thresholds are host memory in both entry points.  The workspace is the context's fourth (next to the
 * hazard's, the footprint's and the loss's): calls of tcr_rainfall_* on one context must be ordered, but one may be in flight next
 * to a tcr_hazard_*, tcr_windfield_* or tcr_loss_* call on another stream. */
#define TCR_RAIN_TOTAL 0
#define TCR_RAIN_PEAK_RATE 1
typedef struct {
    double dt_s, r_out_km, v_lo_kt, v_hi_kt;
    double a[4], b[4];                     /* T0, Tm, rm, re = a[i] + b[i] U */
    int32_t substeps, stat;
} tcr_rain_params;
int tcr_rainfall_dev(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, const tcr_rain_params *prm, int64_t n_site, const double *site_lon,
                     const double *site_lat, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_value, void *stream);
int tcr_rainfall_host(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, const tcr_rain_params *prm, int64_t n_site, const double *site_lon,
                      const double *site_lat, int32_t n_bin, const double *thresholds, int32_t *counts, double *site_value);
/* (site, record) pairs the last tcr_rainfall_* call of this context evaluated after culling; waits for that call */
int tcr_rainfall_pairs(tcr_ctx *ctx, int64_t *pairs);

/* ---- compound hazard: joint exceedance of footprint wind and storm rain at sites ------------------------------------- */
/* replaces: nothing in the reference's code; the compound event behind flood-plus-wind exposure, outage models and parametric
 * covers: how many storms bring a site a wind of at least u AND a rain of at least p.  The count needs both values of every
 * (site, storm) pair at once, so both footprints are evaluated in one scan and the joint histogram is built there; the
 * [n_site][n_trk] planes are optional outputs.
 *   track           a storm's leading run of samples where all eight planes are finite: the seven of tcr_wind_tracks and vmax
 *                   [n_trk][row_stride] (the rainfall's third plane).  Records and sub-steps as in both sections above.
 *   W, site_wind    what tcr_windfield_* writes to site_max on that track with `wind`;  P, site_rain: what tcr_rainfall_* writes
 *                   to site_value on (lon, lat, vmax) cut to that track with `rain` (stat TCR_RAIN_TOTAL or TCR_RAIN_PEAK_RATE).
 *                   Both [n_site][n_trk], optional (NULL: not written).  A record counts for each hazard under that hazard's own
 *                   r_out_km, so W can be NaN where P is not.  On storms whose eight planes are finite over the track the seven
 *                   (or three) give, W and P are bit for bit the two entry points' outputs.
 *   kw, kr          the number of wind_thresholds <= W and of rain_thresholds <= P; 0 for a NaN.
 *   counts          [n_site][n_group][n_wbin + 1][n_rbin + 1] (int32): storms of the group with kw >= a and kr >= b.  Index 0 on
 *                   an axis is "no condition on this hazard": counts[..][1:][0] are the wind footprint's counts, counts[..][0][1:]
 *                   the rainfall's, counts[..][1:][1:] the joint (AND) table and counts[..][0][0] the size of the group.  The OR
 *                   table follows by inclusion-exclusion: wind + rain - and.
 * Arguments: those of tcr_windfield_* and of tcr_rainfall_* under the same rules, each list of thresholds under the rule of its own
 * entry point, and wind->dt_s == rain->dt_s, wind->substeps == rain->substeps, (n_wbin + 1) (n_rbin + 1) <= 64.  Every message
 * begins with "tcr_compound:".  rm > 0 and finite at every sample of a track: tcr_compound_host checks the rmax_km plane as
 * tcr_windfield_host does; tcr_compound_dev cannot, and drops a storm with a bad rm (NaN on both planes at every site, counted
 * only at index 0 of both axes).  Results are a max of per-pair values, a sum of one accumulator in record order and integer
 * counts: bit-identical from run to run, whatever the launch shape, the site order or the storm order.  _dev: planes, vmax,
 * sites, counts, site_wind and site_rain are device memory, asynchronous on `stream`; group_off and both threshold lists are host
 * memory in both entry points.  The workspace is the context's fifth: calls of tcr_compound_* on one context must be ordered, but
 * one may be in flight next to a tcr_hazard_*, tcr_windfield_*, tcr_loss_* or tcr_rainfall_* call on another stream. */
int tcr_compound_dev(tcr_ctx *ctx, const tcr_wind_tracks *tracks, const double *vmax, const tcr_wind_params *wind,
                     const tcr_rain_params *rain, int64_t n_site, const double *site_lon, const double *site_lat, int32_t n_wbin,
                     const double *wind_thresholds, int32_t n_rbin, const double *rain_thresholds, int32_t *counts, double *site_wind,
                     double *site_rain, void *stream);
int tcr_compound_host(tcr_ctx *ctx, const tcr_wind_tracks *tracks, const double *vmax, const tcr_wind_params *wind,
                      const tcr_rain_params *rain, int64_t n_site, const double *site_lon, const double *site_lat, int32_t n_wbin,
                      const double *wind_thresholds, int32_t n_rbin, const double *rain_thresholds, int32_t *counts, double *site_wind,
                      double *site_rain);
/* (site, record) pairs the last tcr_compound_* call of this context evaluated after culling with the larger radius; waits for it */
int tcr_compound_pairs(tcr_ctx *ctx, int64_t *pairs);

/* ---- wind duration: hours at or above wind levels at sites ------------------------------------------------------------ */
/* replaces: nothing in the reference's code; the "for how long" next to the footprint's "how strong": hours of gale-, storm- and
 * hurricane-force wind per storm and per year, which downtime and outage models, parametric covers and fatigue-type damage work
 * from.  The footprint's wind is evaluated once per (site, record) pair and time is accumulated for up to 8 levels at once.
 *   track, records, sub-steps, inclusion and the wind of a (site, record) pair: those of the wind footprint above, bit for bit.
 *                   The value compared with a level is the very double tcr_windfield_* takes the max of.
 *   levels          n_level wind levels (m/s), 1 <= n_level <= 8, finite, > 0, strictly ascending.
 *   weights         record q of a storm's n_rec records carries the half-weight h_q = 2, or 1 for q = 0 and q = n_rec - 1: the
 *                   trapezoid rule in units of half a sub-step.  u = dt_s / (7200 substeps) is the hours per half-weight.
 *   H[l][i][s]      the int32 sum of h_q over the included records of storm s at site i whose wind is >= levels[l].
 *                   n_rec <= 2^26, so H < 2^28.
 *   site_hours      a host array of n_level device pointers (host pointers in tcr_duration_host); the array may be NULL, and so may
 *                   any entry (not written).  Entry l is a [n_site][n_trk] plane: (double)H[l][i][s] * u (one multiply); NaN where
 *                   no record of the storm is included at the site (so at every level alike), 0.0 where records are included but
 *                   none reaches the level.
 *   counts          [n_site][n_group][n_level][n_bin] (int32): storms s in [group_off[g], group_off[g + 1]) with
 *                   (double)H * u >= thresholds[b] (hours).  A NaN counts nowhere.
 *   half_steps      [n_site][n_group][n_level] (int64, optional, NULL: not written): the sum of H over the storms of the group.
 *                   Expected hours per year at or above a level: half_steps summed over the groups, times u / total_years.
 * Arguments: tracks and prm under exactly the rules of tcr_windfield_*; 1 <= n_level <= 8 and the levels as above; thresholds
 * finite, > 0 and strictly ascending; n_level * (n_bin + 1) <= 64.  Every message begins with "tcr_duration:".  rm > 0 and finite
 * at every sample of a track: tcr_duration_host checks the rmax_km plane as tcr_windfield_host does; tcr_duration_dev cannot, and
 * drops a storm with a bad rm (NaN at every site and level, counted nowhere).
 * Not modelled: duration is quantised to dt_s / (2 substeps), and a crossing of a level between two records is not interpolated.
 * Everything accumulated is an integer (that is what the half-weights are for: a sum of fp64 hours would depend on its order), so
 * every output is bit-identical from run to run, whatever the launch shape, the site order, the storm order or the chunking.
 * _dev: planes, sites, counts, half_steps and the planes site_hours points to are device memory, asynchronous on `stream`; levels,
 * thresholds, group_off and the site_hours pointer array are host memory in both entry points.  The workspace is the context's
 * sixth: calls of tcr_duration_* on one context must be ordered, but one may be in flight next to a tcr_hazard_*, tcr_windfield_*,
 * tcr_loss_*, tcr_rainfall_* or tcr_compound_* call on another stream. */
int tcr_duration_dev(tcr_ctx *ctx, const tcr_wind_tracks *tracks, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                     const double *site_lat, int32_t n_level, const double *levels, int32_t n_bin, const double *thresholds,
                     int32_t *counts, int64_t *half_steps, double *const *site_hours, void *stream);
int tcr_duration_host(tcr_ctx *ctx, const tcr_wind_tracks *tracks, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                      const double *site_lat, int32_t n_level, const double *levels, int32_t n_bin, const double *thresholds,
                      int32_t *counts, int64_t *half_steps, double *const *site_hours);
/* (site, record) pairs the last tcr_duration_* call of this context evaluated after culling; waits for that call */
int tcr_duration_pairs(tcr_ctx *ctx, int64_t *pairs);

/* ---- directional wind: peak wind by compass sector at sites ------------------------------------------------------------- */
/* replaces: nothing in the reference's code; the "from where" next to the footprint's "how strong": directional design wind
 * speeds, onshore against offshore wind at a coast, wind-driven rain on a facade, the exposure of a line or a runway.  The
 * footprint's wind vector is formed once per (site, record) pair and its speed goes to the maximum of the compass sector it blows
 * from, for up to 8 equal sectors at once.
 *   track, records, sub-steps, inclusion and the wind of a (site, record) pair: those of the wind footprint above, bit for bit.
 *   h               +1 for a centre latitude >= 0, -1 otherwise (from the sign of the record's sin lat: latitudes in
 *                   (-28 * 2^-1074, 0), whose radians round to zero, take +1).
 *   d, g, w         (d_e, d_n) = (e, n) / |(e, n)|, the footprint's own e and n: the unit bearing from the centre to the site.
 *                   g_e = h (-d_n + be / 2), g_n = h (d_e + bn / 2) with b = 2 h A / v;  w = V (g_e, g_n).  |w| is the footprint's
 *                   double, V sqrt(1 + |A / v|^2 + d_e b_n - d_n b_e), the one tcr_windfield_* takes the max of.
 *   theta           the bearing of (-w_e, -w_n) in degrees clockwise from north, in [0, 360): the direction the wind blows from.
 *   sectors         n_sector equal sectors of W = 360 / n_sector degrees, 1 <= n_sector <= 8; sector k holds the pairs with
 *                   theta - sector0_deg in [(k - 1/2) W, (k + 1/2) W) mod 360.  With n_sector = 8 and sector0_deg = 0: 0 N, 1 NE,
 *                   2 E, ... 7 NW.  A pair with |w| == 0 (the site on the centre, where (e, n) = 0; the profile clamped at 0 far
 *                   out; v <= 0) has no sector and adds nothing.  The sector is decided from the signs of the cross products of
 *                   (-w_e, -w_n) with the boundaries' unit vectors, not from a rounded angle: a pair within rounding of a
 *                   boundary falls to one of its two sectors, and every other pair to its own.
 *   site_dir_max    a host array of n_sector device pointers (host pointers in tcr_directional_host); the array may be NULL, and so
 *                   may any entry (not written).  Entry k is a [n_site][n_trk] plane: max(0, max of |w| over the storm's included
 *                   pairs of sector k); NaN in every sector where no record of the storm is included at the site, 0.0 in a sector
 *                   no wind came from (the storm reached the site and did not exceed there).  The max over the sectors is
 *                   tcr_windfield_*'s site_max bit for bit; with n_sector = 1 the plane is site_max.
 *   counts          [n_site][n_group][n_sector][n_bin] (int32): storms s in [group_off[g], group_off[g + 1]) with
 *                   site_dir_max[k] >= thresholds[b].  A NaN counts nowhere.
 * Arguments: tracks and prm under exactly the rules of tcr_windfield_*; 1 <= n_sector <= 8; sector0_deg finite and in [0, 360);
 * thresholds finite and strictly ascending; n_sector * (n_bin + 1) <= 64.  Every message begins with "tcr_directional:".  rm > 0 and
 * finite at every sample of a track: tcr_directional_host checks the rmax_km plane as tcr_windfield_host does; tcr_directional_dev
 * cannot, and drops a storm with a bad rm (NaN at every site and sector, counted nowhere).
 * Results are maxima of per-pair values and integer counts: bit-identical from run to run, whatever the launch shape, the site
 * order or the storm order.  _dev: planes, sites, counts and the planes site_dir_max points to are device memory, asynchronous on
 * `stream`; thresholds, group_off and the site_dir_max pointer array are host memory in both entry points.  The workspace is the
 * context's eighth: calls of tcr_directional_* on one context must be ordered, but one may be in flight next to a call of any
 * other analysis on another stream. */
int tcr_directional_dev(tcr_ctx *ctx, const tcr_wind_tracks *tracks, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                        const double *site_lat, int32_t n_sector, double sector0_deg, int32_t n_bin, const double *thresholds,
                        int32_t *counts, double *const *site_dir_max, void *stream);
int tcr_directional_host(tcr_ctx *ctx, const tcr_wind_tracks *tracks, const tcr_wind_params *prm, int64_t n_site, const double *site_lon,
                         const double *site_lat, int32_t n_sector, double sector0_deg, int32_t n_bin, const double *thresholds,
                         int32_t *counts, double *const *site_dir_max);
/* (site, record) pairs the last tcr_directional_* call of this context evaluated after culling; waits for that call */
int tcr_directional_pairs(tcr_ctx *ctx, int64_t *pairs);

/* ---- rain accumulation windows: peak D-hour rain depth at sites ------------------------------------------------------- */
/* replaces: nothing in the reference's code; what lies between the rainfall footprint's two statistics.  The storm total is the
 * rain of a window longer than the track, the peak rate that of a window of no length; flood and drainage work needs the largest
 * depth in any 6, 12, 24 or 72 consecutive hours, and its return levels: the depth-duration-frequency table of a site.  The
 * hourly series of every (site, storm) pair is far too large to store, so the window maximum is formed inside the scan, for up
 * to 8 window lengths at once.
 *   track, records, sub-steps, inclusion and the rate of a (site, record) pair: those of the rainfall footprint above, bit for bit
 *                   (n samples, nr = (n - 1) substeps + 1 records).
 *   h               dt_s / (3600 substeps) hours.
 *   rho_q           the rate (mm/h) of record q at the site if the pair is included (r <= r_out_km), else 0.
 *   I_q             (h / 2) (rho_q + rho_q+1), q = 0 .. nr - 2: the trapezoid of one sub-interval.
 *   T_k             the sum of I_q over q < k substeps, added in ascending q; T_0 = 0.  The depth up to sample k = 0 .. n - 1.
 *   windows         n_window lengths m_i in samples (window_samples, int32), 1 <= n_window <= 8, 1 <= m_i <= 96, strictly ascending.
 *   A_i             max over k = 0 .. n - 1 of T_k - T_max(k - m_i, 0)   (mm).
 *   site_window     a host array of n_window device pointers (host pointers in tcr_accumulation_host); the array may be NULL, and
 *                   so may any entry (not written).  Entry i is a [n_site][n_trk] plane of A_i; NaN where no record of the storm
 *                   is included at the site (so in every window alike).  It can be 0.0.
 *   counts          [n_site][n_group][n_window][n_bin] (int32): storms s in [group_off[g], group_off[g + 1]) with
 *                   A_i >= thresholds[b] (mm).  A NaN counts nowhere.
 * Consequences: windows start and end on track samples (sub-steps refine the integral inside a sample interval, not the window's
 * position).  A window of m_i >= n - 1 samples gives T_n-1, the storm total by the trapezoid rule of TCR_RAIN_TOTAL, equal to it
 * up to the rounding of the two summations.  A_i is non-decreasing in m_i exactly, also in floating point (T is a non-decreasing
 * sequence and subtraction is monotone), and A_i <= m_i (dt_s / 3600) times the peak rate of TCR_RAIN_PEAK_RATE.
 * Arguments: tracks and prm under exactly the rules of tcr_rainfall_*, and prm->stat == TCR_RAIN_TOTAL; the windows as above;
 * n_window * (n_bin + 1) <= 64; 512 (m_max + 1) + 256 n_window (n_bin + 1) <= 65536, the LDS bytes of a wave (m_max: the longest
 * window).  Every message begins with "tcr_accumulation:" and nothing is launched after one.
 * Not modelled: window positions between samples; rain asymmetry and decay after landfall, as in the rainfall footprint.
 * T of a (site, storm) is one accumulator over the included records in record order, whatever else the call holds (the terms of
 * records that are not included are exact zeros, so skipping them changes no bits), a window's value is a difference and a max
 * of such sums and the counts are integers: every output is bit-identical from run to run, whatever the launch shape, the site
 * order or the storm order.  _dev: planes, sites, counts and the planes site_window points to are device memory, asynchronous on
 * `stream`; window_samples, thresholds, group_off and the site_window pointer array are host memory in both entry points.  The
 * workspace is the context's seventh: calls of tcr_accumulation_* on one context must be ordered, but one may be in flight next
 * to a call of any other analysis, tcr_rainfall_* included, on another stream. */
int tcr_accumulation_dev(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, const tcr_rain_params *prm, int64_t n_site,
                         const double *site_lon, const double *site_lat, int32_t n_window, const int32_t *window_samples, int32_t n_bin,
                         const double *thresholds, int32_t *counts, double *const *site_window, void *stream);
int tcr_accumulation_host(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, const tcr_rain_params *prm, int64_t n_site,
                          const double *site_lon, const double *site_lat, int32_t n_window, const int32_t *window_samples, int32_t n_bin,
                          const double *thresholds, int32_t *counts, double *const *site_window);
/* (site, record) pairs the last tcr_accumulation_* call of this context evaluated after culling; waits for that call */
int tcr_accumulation_pairs(tcr_ctx *ctx, int64_t *pairs);

/* ---- closest approach: passage distance, time, intensity, motion and side at sites -------------------------------------- */
/* replaces: nothing in the reference's code; the "how did it pass" next to the other analyses' "how strong".  Every other per-site
 * analysis reduces a storm to one extreme at a site; this one keeps the geometry of the passage: the frequency of passages by
 * distance band and intensity (the statistic behind "hurricanes passing within 50 nmi", the joint-probability method of coastal
 * surge work, siting studies) and the per-storm parameters at the closest point of approach (CPA).
 *   tracks          tcr_hazard_tracks (lon, lat, vmax, groups).  A storm's track is the samples before the first with a non-finite
 *                   lon, lat or vmax; a track of fewer than 2 samples has no records.
 *   rm              rmax_km: an optional [n_trk][row_stride] plane (km); prm->rmax_const_km > 0: that value everywhere; both NULL /
 *                   0 (tcr_windfield_*'s rules): Willoughby et al. (2006), 46.4 exp(-0.0155 v + 0.0169 |lat|) km at every sample.
 *                   A track with an rm that is not finite and > 0 at one of its samples has no records.
 *   records         (n - 1) substeps + 1 per storm of n samples: the samples, and substeps - 1 sub-samples between neighbours, as
 *                   the wind footprint's: dl = lon_k+1 - lon_k, dl -= 360 floor((dl + 180) / 360) (the short way round), and lon,
 *                   lat, v and rm linear in tau = j / substeps.
 *   motion          of a record: that of the segment [k, k + 1] it lies on; the track's last record takes the last segment's.
 *                   With dl wrapped as above, phim = (lat_k + lat_k+1) / 2 and Re = 6.3781e6 m:
 *                   ue = Re cos(phim) rad(dl) / dt_s, un = Re rad(lat_k+1 - lat_k) / dt_s, speed = sqrt(ue^2 + un^2),
 *                   heading = atan2(ue, un) in degrees, mapped to [0, 360); NaN when ue == un == 0.
 *   CPA             per (site, storm), over the records with haversine argument q = sin^2(dphi / 2) + cos phi1 cos phi2
 *                   sin^2(dlam / 2) <= a_R = sin^2(band_km[n_band - 1] / (2 Re / 1000)): the record of least q; on equal q the
 *                   earliest.  Taken on the records: the minimum along the chord between two records is not modelled, substeps
 *                   is the refinement.
 *   planes          a host array of 7 device pointers (host pointers in tcr_approach_host); the array may be NULL, and so may any
 *                   entry (not written).  Entry k is a [n_site][n_trk] plane of the CPA record's (NaN in every plane when the storm
 *                   has no included record):
 *                     0 distance_km  (Re / 1000) 2 asin(sqrt(q))
 *                     1 time_h       (double)index * (dt_s / (3600 substeps)): hours since the track's first sample
 *                     2 v            intensity (m/s)
 *                     3 speed        forward speed (m/s)
 *                     4 heading_deg  as above
 *                     5 side_km      +distance when the site is to the right of the motion, -distance to the left, 0.0 when
 *                                    undefined.  With (e, nn) the centre -> site direction of the wind footprint
 *                                    (e = cos phis sin dlam, nn = cos phic sin phis - sin phic cos phis cos dlam) and
 *                                    cross = ue nn - un e: right when cross < 0, left when cross > 0, undefined when cross == 0
 *                                    (the site on the centre, a stationary segment)
 *                     6 rmax_km      rm
 *   counts          [n_site][n_group][n_band][n_bin] (int32): storms s in [group_off[g], group_off[g + 1]) with distance_km <=
 *                   band_km[band] and v >= thresholds[bin].  The band test is made on the very double written to plane 0, so the
 *                   counts are an exact function of planes 0 and 2.
 * Arguments: dt_s finite and > 0; substeps in [1, 64]; rmax_const_km finite and >= 0, and 0 when rmax_km is given; 1 <= n_band <= 8
 * bands, finite, > 0, strictly ascending and at most 5000 km; thresholds finite and strictly ascending; n_band * (n_bin + 1) <= 64;
 * 1 <= n_t <= 2^20.  Every message begins with "tcr_approach:".
 * One lane owns a (site, storm), its records arrive in record order and culling never removes an included record, so the argmin
 * and its tie rule, and with them every output, are bit-identical from run to run, whatever the launch shape, the site order, the
 * storm order or the chunking.  _dev: planes, rmax_km, sites, counts and the planes `planes` points to are device memory,
 * asynchronous on `stream`; band_km, thresholds, group_off and the pointer array are host memory in both entry points.  The workspace
 * is the context's ninth: calls of tcr_approach_* on one context must be ordered, but one may be in flight next to a call of any
 * other analysis on another stream. */
#define TCR_APPROACH_PLANES 7
typedef struct {
    double dt_s;                 /* sample spacing (s) */
    int32_t substeps;            /* records per sample interval, 1 .. 64 */
    double rmax_const_km;        /* > 0: rm everywhere; 0: the rmax_km plane, or Willoughby et al. (2006) without one */
} tcr_approach_params;
int tcr_approach_dev(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, const double *rmax_km, const tcr_approach_params *prm,
                     int64_t n_site, const double *site_lon, const double *site_lat, int32_t n_band, const double *band_km,
                     int32_t n_bin, const double *thresholds, int32_t *counts, double *const *planes, void *stream);
int tcr_approach_host(tcr_ctx *ctx, const tcr_hazard_tracks *tracks, const double *rmax_km, const tcr_approach_params *prm,
                      int64_t n_site, const double *site_lon, const double *site_lat, int32_t n_band, const double *band_km,
                      int32_t n_bin, const double *thresholds, int32_t *counts, double *const *planes);
/* (site, record) pairs the last tcr_approach_* call of this context evaluated after culling; waits for that call */
int tcr_approach_pairs(tcr_ctx *ctx, int64_t *pairs);

/* ---- row selection (return levels): the k-th largest value of every row of a per-storm plane ----------------------------- */
/* replaces: nothing in the reference's code; the inverse of the return periods above.  With return_period = total_years /
 * count(peak >= v), the level of period T at a site is the k-th largest storm peak there, k the smallest integer with
 * k T >= total_years: an order statistic of the site's row of site_max / site_value, taken while the plane is on the device.
 *   plane           [n_row][row_stride] fp64, of which the first n_col values of a row are the row; NaN is "absent".
 *   order           that of the key of a double: its bits, every bit flipped for a negative, the sign bit flipped otherwise, as an
 *                   unsigned integer: -inf < negatives < -0.0 < +0.0 < positives < +inf.  A NaN of either sign has no place in it.
 *   level           [n_row][n_rank]: level[r][j] is the ranks[j]-th largest value of row r that is not NaN, one of the row's own
 *                   values bit for bit (no arithmetic touches a value); NaN when the row holds fewer such values.
 *   n_valid         [n_row] (int32, optional, NULL: not written): how many values of the row are not NaN.
 * Arguments: n_row >= 0, 1 <= n_col <= 2^31 - 1, row_stride >= n_col, 1 <= n_rank <= TCR_SELECT_MAX_RANKS, ranks >= 1 in any order,
 * repeats allowed.  Every message begins with "tcr_select:" and nothing is launched after one.
 * One workgroup per row compacts the keys of the row's non-NaN values into LDS in one pass; a row with at most
 * TCR_SELECT_LDS_KEYS of them is selected there, a longer one from the row in global memory, by the same radix selection (8-bit
 * digits from the top, all ranks together).  The result is a function of the row's multiset of values alone: bit-identical from
 * run to run, on both paths, and whatever the order of the values.  _dev: plane, level and n_valid are device memory,
 * asynchronous on `stream`; ranks is host memory in both entry points.  No workspace: calls on one context need no ordering. */
#define TCR_SELECT_LDS_KEYS 8192      /* keys a row may hold in LDS; rows with more take the global path */
#define TCR_SELECT_MAX_RANKS 64
int tcr_select_dev(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, int32_t n_rank,
                   const int64_t *ranks, double *level, int32_t *n_valid, void *stream);
int tcr_select_host(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, int32_t n_rank,
                    const int64_t *ranks, double *level, int32_t *n_valid);

/* ---- row tail fit (return levels past the record): a generalized Pareto tail on the k largest values of every row ---------- */
/* replaces: nothing in the reference's code.  Row selection stops at T = total_years, and its last order statistics are single
 * storms; this is the standard peaks-over-threshold step on the same plane: per row, a generalized Pareto distribution (GPD)
 * fitted to the excesses of the k largest values over the (k+1)-th, and the level of any return period read off the fit.
 * For one row of a [n_row][n_col] fp64 plane, with k exceedances (2 <= k <= TCR_TAIL_MAX_K = 2048), total_years > 0 and return
 * periods T_j (1 to 64 of them, finite, > 0):
 *   1. n_valid is the number of values that are not NaN, in tcr_select's key order.  If n_valid < k + 1, the fit is undefined.
 *   2. u is the (k+1)-th largest value, bit for bit one of the row's own.  The sample is the k largest values.  Ties at u are
 *      included until there are k; they have excess +0.0.
 *   3. Excesses are y_1 <= ... <= y_k, with y_i = x_i - u taken after sorting ascending.
 *   4. Two sums are formed with a fixed tree.  Pad to P with +0.0, where P is the next power of two >= k.  Then repeat
 *      s[i] = s[2i] + s[2i+1] until one value is left.
 *        S0 = tree(y_i)
 *        S1 = tree((double)(k - i) * y_i), with i 1-based
 *        a0 = S0 / k
 *        a1 = S1 / ((double)k * (double)(k - 1))
 *   5. d = a0 - 2.0 * a1.  The fit is defined iff d > 0 and a1 > 0.  An Inf or NaN among the excesses fails this by itself.
 *      These are the Hosking & Wallis (1987) probability-weighted-moment (PWM) estimators:
 *        xi = 2.0 - a0 / d
 *        sigma = 2.0 * a0 * a1 / d, evaluated as ((2.0 * a0) * a1) / d
 *   6. L_j = log((k / total_years) * T_j) is computed once on the host in fp64.  The level is NaN when L_j < 0, because T is then
 *      shorter than the threshold's own return period and return_level is the answer there.  Otherwise:
 *        level_j = u + sigma * L_j when xi == 0
 *        level_j = u + sigma * expm1(xi * L_j) / xi otherwise
 *   7. Undefined fit: xi, sigma and all levels are NaN.  u is still reported when n_valid >= k + 1, NaN otherwise.  n_valid is
 *      always reported.
 * Nothing is clamped.  xi <= 1 follows from 2 a1 <= a0 for ascending non-negative excesses.
 * The translation unit is built with -ffp-contract=off.  Steps 1 to 5 are IEEE adds, multiplies, divides and exact int
 * conversions in a stated order, so u, xi and sigma are a function of the row's multiset of values alone, bit for bit; only step
 * 6 goes through log and expm1.
 *   plane, n_row, n_col, row_stride: as tcr_select_*.      periods   [n_period] fp64, host memory in both entry points.
 *   param           [n_row][3]: u, xi, sigma.              level     [n_row][n_period].
 *   n_valid         [n_row] (int32, optional, NULL: not written).
 * Arguments: tcr_select's rules for the plane; 2 <= k <= TCR_TAIL_MAX_K, total_years finite and > 0,
 * 1 <= n_period <= TCR_SELECT_MAX_RANKS, periods finite and > 0.  Every message begins with "tcr_tail:" and nothing is launched
 * after one.  n_row == 0 returns 0.  One workgroup per row: tcr_select's compaction and its selection of rank k + 1 (from LDS or
 * from the row, as there), a gather of the values above u, a bitonic sort in LDS, the sums and the levels.  _dev: plane, param,
 * level and n_valid are device memory, asynchronous on `stream`.  No workspace: calls on one context need no ordering. */
#define TCR_TAIL_MAX_K 2048
int tcr_tail_dev(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, int32_t k, double total_years,
                 int32_t n_period, const double *periods, double *param, double *level, int32_t *n_valid, void *stream);
int tcr_tail_host(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, int32_t k, double total_years,
                  int32_t n_period, const double *periods, double *param, double *level, int32_t *n_valid);

/* ---- row packing (event footprints): the entries of every row of a per-storm plane at or above a floor, as CSR ------------- */
/* replaces: nothing in the reference's code.  Every site analysis above answers a question per site, summed over storms; this is
 * the event set itself: which storm put how much wind or rain on which site, for the block of sites whose plane is on the device.
 *   plane           [n_row][row_stride] fp64, of which the first n_col values of a row are the row.
 *   kept            entry (r, c) is kept iff plane[r][c] >= min_value as an IEEE comparison, the comparison of `counts`
 *                   (site_max >= thresholds[b]): a NaN of either sign is never kept, -0.0 >= 0.0 is true, and min_value = -inf
 *                   keeps every value that is not NaN.
 *   row_ptr         [n_row + 1] int64: row_ptr[0] = 0, row_ptr[r + 1] - row_ptr[r] the number of kept entries of row r,
 *                   row_ptr[n_row] their number nnz.
 *   col, val        [nnz] int32 and fp64: the kept entries of row r in ascending column order at positions row_ptr[r] ...; val is
 *                   a bit copy (no arithmetic touches a value: a kept -0.0 stays -0.0).
 * The result is a function of the plane and min_value alone: bit-identical from run to run and whatever the launch shape (a
 * position is computed from ballots and sums, never handed out by an atomic).
 * Arguments: tcr_select's rules for the plane (n_row >= 0, 1 <= n_col <= 2^31 - 1, row_stride >= n_col); min_value must not be
 * NaN; capacity >= 0.  Every message begins with "tcr_rowpack:" and nothing is launched after one.  n_row == 0 writes
 * row_ptr[0] = 0 and returns 0.
 *   tcr_rowpack_count_dev   writes row_ptr (one workgroup per row counts, one workgroup sums in place).  Counting is a call of
 *                           its own because the caller sizes col / val from row_ptr[n_row] between the two: the one host read
 *                           of the pass.
 *   tcr_rowpack_fill_dev    writes col and val of the first `capacity` entries from the row_ptr the count gave.  It never writes
 *                           at or past capacity, whatever row_ptr says: an entry whose position is not in [0, capacity) is
 *                           dropped.  It cannot report that; it guarantees the bound, and that the first capacity entries are
 *                           the right ones.  capacity == 0: col and val may be NULL.
 *   tcr_rowpack_host        everything in host memory.  capacity == 0 and col == val == NULL: counts only.  Otherwise it fills
 *                           row_ptr and then fails ("capacity") when nnz > capacity, with col / val untouched.
 * _dev: plane, row_ptr, col and val are device memory, asynchronous on `stream`.  No workspace (the scan works in row_ptr itself):
 * calls on one context need no ordering.  A turn of a row's workgroup covers 256 x TCR_ROWPACK_UNROLL columns. */
#define TCR_ROWPACK_UNROLL 8          /* loads a lane has in flight: a workgroup of 256 threads takes 2048 columns per turn */
int tcr_rowpack_count_dev(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, double min_value,
                          int64_t *row_ptr, void *stream);
int tcr_rowpack_fill_dev(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, double min_value,
                         const int64_t *row_ptr, int64_t capacity, int32_t *col, double *val, void *stream);
int tcr_rowpack_host(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, double min_value,
                     int64_t *row_ptr, int64_t capacity, int32_t *col, double *val);

/* ---- joint hazard (co-exceedance between sites): one bit per (row, level, unit), and popcounts of ANDed bit rows -------------- */
/* replaces: nothing in the reference's code.  Every site analysis above treats sites one at a time; this says whether two sites
 * are hit by the same storm, or in the same year: joint[i][j] = the number of units (storms, or years) that reached a level at
 * site i and at site j.  A site analysis writes its per-storm plane for a block of sites; the plane becomes one bit per (site,
 * level, unit) while it is on the device, and the counts are popcounts of ANDed bit rows.  Every result is an integer.
 *   plane           [n_row][row_stride] fp64, of which the first n_col values of a row are the row (tcr_select's rules).
 *   level           [n_row][n_level] fp64, not NaN, per row (an absolute threshold is the same value in every row).
 *   reaches         column c of row r reaches level l iff plane[r][c] >= level[r][l] as an IEEE comparison, the comparison of
 *                   `counts` and of tcr_rowpack: a NaN of either sign never reaches, -0.0 >= 0.0 reaches, +inf as a level admits
 *                   only +inf, -inf admits every value that is not NaN.
 *   unit            unit_of == NULL: unit = column, one bit per storm, n_unit = n_col.  Otherwise unit_of [n_col] int32 in
 *                   [0, n_unit), and bit u is set iff ANY column with unit_of[c] == u reaches the level ("both sites exceeded in
 *                   the same season").  The mapping is arbitrary: it need not be sorted, and units may be empty.
 *   bits            bits[l * level_stride + r * n_word + (u >> 6)] is a uint64 whose bit u & 63 is unit u, n_word =
 *                   ceil(n_unit / 64).  Bits at or past n_unit in the last word of a row are zero.  level_stride is in words and
 *                   >= n_row * n_word; it may be that of a larger table of n_row_total rows (level_stride >= n_row_total * n_word)
 *                   into which a block of rows is packed by passing bits + first_row * n_word.
 *   n_set           [n_level][n_set_stride] int32 (n_set_stride >= n_row), or NULL: n_set[l][r] = the popcount of row r at level l.
 *   counts          tcr_joint_cross_dev: [n_level][n_a][n_b] int32, counts[l][i][j] = sum over w of popcount(a[l][i][w] &
 *                   b[l][j][w]).  a_bits == b_bits is allowed (the full square is computed; its diagonal is n_set).
 * The results are functions of the inputs alone: a word is a ballot or an OR of bits, a count a sum of integers.  No
 * floating-point atomics and no global atomics are used.
 * Limits: 1 <= n_level <= TCR_JOINT_MAX_LEVELS; n_col in [1, 2^31 - 1]; with unit_of, 1 <= n_unit <= TCR_JOINT_MAX_MAPPED_UNITS,
 * without it n_unit == n_col.  tcr_joint_cross_dev: n_a <= 65535 x 64, n_b < 2^30, n_word <= 2^25.  Every message begins with
 * "tcr_joint:" and nothing is launched after one.  n_row == 0 (n_a == 0 or n_b == 0) does nothing and returns 0.
 *   tcr_joint_pack_dev    plane, level, unit_of, bits and n_set are device memory, asynchronous on `stream`.  It cannot look at
 *                         the entries of level or unit_of: a NaN level is reached by nothing, and a column whose unit_of is not
 *                         in [0, n_unit) sets no bit.  Without unit_of one workgroup per row makes the ballots of 64 adjacent
 *                         columns the words, all levels on one load of the plane; with it the hits of a row are ORed into an
 *                         image of the row in LDS, for as many levels at a time as 4096 words hold.
 *   tcr_joint_cross_dev   a_bits, b_bits and counts are device memory.  One workgroup per 64 x 64 tile of counts[l] walks the
 *                         words in chunks of TCR_JOINT_KW.
 *   tcr_joint_host        everything in host memory: uploads the plane, packs it and crosses the table with itself, counts
 *                         [n_level][n_row][n_row], n_set [n_level][n_row] or NULL.  It also checks the entries of level (NaN) and
 *                         of unit_of (range).  For the ABI-only user and for tests: when plane, table and counts together exceed
 *                         2^32 bytes it fails with a message ("too large for tcr_joint_host") before anything is allocated.
 * No workspace: calls on one context need no ordering. */
#define TCR_JOINT_MAX_LEVELS 16
#define TCR_JOINT_MAX_MAPPED_UNITS 262144      /* 2^18: one level of a mapped row is 4096 words of LDS */
#define TCR_JOINT_KW 32               /* words of a bit row a workgroup of tcr_joint_cross_dev stages per chunk: 2 x 16.5 KB of LDS */
int tcr_joint_pack_dev(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, const double *level,
                       int32_t n_level, const int32_t *unit_of, int64_t n_unit, uint64_t *bits, int64_t level_stride, int32_t *n_set,
                       int64_t n_set_stride, void *stream);
int tcr_joint_cross_dev(tcr_ctx *ctx, const uint64_t *a_bits, int64_t n_a, int64_t a_level_stride, const uint64_t *b_bits, int64_t n_b,
                        int64_t b_level_stride, int64_t n_word, int32_t n_level, int32_t *counts, void *stream);
int tcr_joint_host(tcr_ctx *ctx, const double *plane, int64_t n_row, int64_t n_col, int64_t row_stride, const double *level,
                   int32_t n_level, const int32_t *unit_of, int64_t n_unit, int32_t *counts, int32_t *n_set);

#ifdef __cplusplus
}
#endif
#endif /* TCRISK_HIP_H */
