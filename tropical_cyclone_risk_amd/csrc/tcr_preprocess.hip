// Environment preprocessing behind the ABI: potential intensity, chi / rh_mid (tcr_thermo.hip) and the monthly wind
// statistics (tcr_prep.hip).  The entropy table they read is staged by tcr_entropy_table_upload (tcr_stage.hip).
#pragma once
#include "tcr_integrate.hip"               // timing_events

namespace {

template <typename T>
int wind_stats_dev_impl(tcr_ctx *ctx, int64_t n_samples, int64_t n_points, const T *const wnd[4],
                        const int32_t *day_start, int32_t n_days, double *out, void *stream_)
{
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    if (!wnd || !out || n_samples <= 0 || n_points <= 0) return fail(ctx, "tcr_wind_stats_dev: bad argument");
    if (!day_start) n_days = (int32_t)n_samples;
    if (n_days < 2) return fail(ctx, "tcr_wind_stats_dev: a covariance needs at least two days");
    WindStatArgsT<T> a{};
    for (int c = 0; c < 4; ++c) a.w[c] = wnd[c];
    a.day_start = day_start; a.n_days = n_days; a.n_points = n_points; a.out = out;
    hipEvent_t *ev = nullptr;
    if (ctx->tr.timing && timing_events(ctx, &ev)) return -1;
    if (ev) { HIPCHK(ctx, hipEventRecord(ev[0], st)); HIPCHK(ctx, hipEventRecord(ev[1], st)); }
    hipLaunchKernelGGL(k_wind_stats<T>, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, st, a);
    if (ev) { HIPCHK(ctx, hipEventRecord(ev[2], st)); HIPCHK(ctx, hipEventRecord(ev[3], st)); HIPCHK(ctx, hipEventRecord(ev[4], st)); HIPCHK(ctx, hipEventRecord(ev[5], st)); }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

template <typename T>
int wind_stats_host_impl(tcr_ctx *ctx, int64_t n_samples, int64_t n_points, const T *const wnd[4],
                         const int32_t *day_start, int32_t n_days, double *out)
{
    if (!enter(ctx)) return -1;
    if (!wnd || !out || n_samples <= 0 || n_points <= 0) return fail(ctx, "tcr_wind_stats_host: bad argument");
    DevBuf B;
    const T *d_w[4];
    for (int c = 0; c < 4; ++c)
        if (!(d_w[c] = B.put(wnd[c], (size_t)n_samples * n_points))) return fail(ctx, "tcr_wind_stats_host: device allocation failed");
    const int32_t *d_ds = nullptr;
    if (day_start && !(d_ds = B.put(day_start, (size_t)n_days + 1))) return fail(ctx, "tcr_wind_stats_host: device allocation failed");
    double *d_out = B.get<double>((size_t)14 * n_points);
    if (!d_out) return fail(ctx, "tcr_wind_stats_host: device allocation failed");
    if (wind_stats_dev_impl<T>(ctx, n_samples, n_points, d_w, d_ds, n_days, d_out, ctx->stream)) return -1;
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, sizeof(double) * 14 * (size_t)n_points, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // namespace

extern "C" {

int tcr_potential_intensity_dev(tcr_ctx *ctx, int64_t n_points, int32_t n_lev, const double *p_env, const double *sst,
                                const double *psl, const double *T_env, const double *r_env, double ck_over_cd,
                                double *pi, void *stream_)
{
    if (!ctx) return -1;
    const Staging &S = ctx->sg;
    if (!S.d_tab.p) return fail(ctx, "tcr_potential_intensity: no entropy table (tcr_entropy_table_upload)");
    if (n_points <= 0 || n_lev < 2 || !p_env || !sst || !psl || !T_env || !r_env || !pi)
        return fail(ctx, "tcr_potential_intensity: bad argument (at least two levels)");
    hipStream_t st = enter(ctx, stream_);
    if (!st) return -1;
    th::PiArgs a{};
    a.tab.np = S.tab_np; a.tab.ns = S.tab_ns;
    a.tab.p = S.d_tab.p; a.tab.s = S.d_tab.p + S.tab_np; a.tab.T = S.d_tab.p + S.tab_np + S.tab_ns;
    a.n_points = n_points; a.n_lev = n_lev; a.p_env = p_env; a.sst = sst; a.psl = psl; a.T_env = T_env; a.r_env = r_env;
    a.cecd = ck_over_cd; a.pi = pi;
    hipLaunchKernelGGL(th::k_potential_intensity, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int tcr_potential_intensity_host(tcr_ctx *ctx, int64_t n_points, int32_t n_lev, const double *p_env, const double *sst,
                                 const double *psl, const double *T_env, const double *r_env, double ck_over_cd, double *pi)
{
    if (!enter(ctx)) return -1;
    if (n_points <= 0 || n_lev < 2) return fail(ctx, "tcr_potential_intensity: bad argument (at least two levels)");
    for (int k = 1; k < n_lev; ++k)
        if (!(p_env[k] < p_env[k - 1])) return fail(ctx, "tcr_potential_intensity: levels must run from the lowest (highest pressure) up");
    DevBuf B;
    const double *d_p = B.put(p_env, (size_t)n_lev), *d_sst = B.put(sst, (size_t)n_points), *d_psl = B.put(psl, (size_t)n_points);
    const double *d_T = B.put(T_env, (size_t)n_lev * n_points), *d_r = B.put(r_env, (size_t)n_lev * n_points);
    double *d_pi = B.get<double>((size_t)n_points);
    if (!d_p || !d_sst || !d_psl || !d_T || !d_r || !d_pi) return fail(ctx, "tcr_potential_intensity_host: device allocation failed");
    if (tcr_potential_intensity_dev(ctx, n_points, n_lev, d_p, d_sst, d_psl, d_T, d_r, ck_over_cd, d_pi, ctx->stream)) return -1;
    HIPCHK(ctx, hipMemcpyAsync(pi, d_pi, sizeof(double) * (size_t)n_points, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int tcr_chi_rh_host(tcr_ctx *ctx, int64_t n_points, const double *sst, const double *psl, const double *T_mid,
                    const double *q_mid, double p_mid, double *chi, double *rh_mid)
{
    if (!enter(ctx)) return -1;
    if (n_points <= 0 || !sst || !psl || !T_mid || !q_mid || !chi || !rh_mid) return fail(ctx, "tcr_chi_rh_host: bad argument");
    DevBuf B;
    const size_t n = (size_t)n_points;
    const double *d_sst = B.put(sst, n), *d_psl = B.put(psl, n), *d_T = B.put(T_mid, n), *d_q = B.put(q_mid, n);
    double *d_chi = B.get<double>(n), *d_rh = B.get<double>(n);
    if (!d_sst || !d_psl || !d_T || !d_q || !d_chi || !d_rh) return fail(ctx, "tcr_chi_rh_host: device allocation failed");
    hipLaunchKernelGGL(th::k_chi_rh, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, ctx->stream, n_points,
                       d_sst, d_psl, d_T, d_q, p_mid, d_chi, d_rh);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(chi, d_chi, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(rh_mid, d_rh, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int tcr_wind_stats_dev(tcr_ctx *ctx, int64_t n_samples, int64_t n_points, const double *const wnd[4],
                       const int32_t *day_start, int32_t n_days, double *out, void *stream_)
{
    return wind_stats_dev_impl<double>(ctx, n_samples, n_points, wnd, day_start, n_days, out, stream_);
}

int tcr_wind_stats_f32_dev(tcr_ctx *ctx, int64_t n_samples, int64_t n_points, const float *const wnd[4],
                           const int32_t *day_start, int32_t n_days, double *out, void *stream_)
{
    return wind_stats_dev_impl<float>(ctx, n_samples, n_points, wnd, day_start, n_days, out, stream_);
}

int tcr_wind_stats_host(tcr_ctx *ctx, int64_t n_samples, int64_t n_points, const double *const wnd[4],
                        const int32_t *day_start, int32_t n_days, double *out)
{
    return wind_stats_host_impl<double>(ctx, n_samples, n_points, wnd, day_start, n_days, out);
}

int tcr_wind_stats_f32_host(tcr_ctx *ctx, int64_t n_samples, int64_t n_points, const float *const wnd[4],
                            const int32_t *day_start, int32_t n_days, double *out)
{
    return wind_stats_host_impl<float>(ctx, n_samples, n_points, wnd, day_start, n_days, out);
}

}  // extern "C"
