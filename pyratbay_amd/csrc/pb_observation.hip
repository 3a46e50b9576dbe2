// Walker-batched retrieval path, the exit towards the sampler: the eclipse factor of a batch whose
// walkers carry a stellar temperature (and optionally a planet radius) of their own, and the
// Gaussian log-likelihood, plain and with per-walker instrumental offsets and uncertainty scaling.
#include "pb_common.h"

namespace {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------
// bandflux[w, b] *= f_dilution[w] (if given), then *= rprs2_w / bandflux_star[w, b]
// (Pyrat.band_integrate, pyrat_obj.py:662-665, with eval()'s tstar branch, pyrat_obj.py:288-294):
// bandflux_star = the band integral of the SED grid interpolated linearly at the walker's stellar
// temperature (spec.flux_interp = interp1d(sed_temps, starflux, axis=0), pyrat/argum.py:93-98).
// Grid (band, walker).  Per sample the interpolated flux is interp1d's linear rule as SciPy states
// it, every operation rounded on its own; the band integral is k_band_integrate_batch's pair loop,
// lane stride and LDS tree with that flux in place of a stored spectrum (the spectra [nw, W] are
// never stored), times the band's height like PassBand.integrate.  A walker whose tstar is NaN or
// outside the grid's temperatures gets +inf in every band.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_star_band_scale_batch(
    double *bandflux, const double *star_grid, const double *sed_temps, const double *tstar,
    double rprs2, const double *rplanet, double rstar, const double *f_dilution, const double *wn,
    const int32_t *band_start, const int32_t *band_count, const double *response,
    const int64_t *response_offset, const double *heights, int nt, int nbands, int nwave)
{
    __shared__ double s_part[kBlock];
    const int b = blockIdx.x, w = blockIdx.y;
    const double t = tstar[w];
    double *out = bandflux + (int64_t)w * nbands + b;
    // (block-uniform: every thread of the block leaves here, before any barrier)
    if (!(t >= sed_temps[0] && t <= sed_temps[nt - 1])) {
        if (threadIdx.x == 0)
            *out = INFINITY;
        return;
    }
    // searchsorted(sed_temps, t, side='left') clipped to [1, nt - 1]
    int hi = 0;
    while (hi < nt && sed_temps[hi] < t)
        hi++;
    hi = min(max(hi, 1), nt - 1);
    const double x_lo = sed_temps[hi - 1];
    const double dx = sed_temps[hi] - x_lo;
    const double dt = t - x_lo;
    const double *y_lo = star_grid + (int64_t)(hi - 1) * nwave;
    const double *y_hi = star_grid + (int64_t)hi * nwave;

    const int start = band_start[b];
    const int count = band_count[b];
    const double *resp = response + response_offset[b];
    double acc = 0.0;
    for (int i = threadIdx.x; i + 1 < count; i += kBlock) {
        const int64_t g = (int64_t)start + i;
        const double s0 = ((y_hi[g] - y_lo[g]) / dx) * dt + y_lo[g];
        const double s1 = ((y_hi[g + 1] - y_lo[g + 1]) / dx) * dt + y_lo[g + 1];
        const double y0 = s0 * resp[i];
        const double y1 = s1 * resp[i + 1];
        acc += 0.5 * (wn[g + 1] - wn[g]) * (y0 + y1);
    }
    s_part[threadIdx.x] = acc;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            s_part[threadIdx.x] += s_part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double star = heights ? s_part[0] * heights[b] : s_part[0];
        double r2 = rprs2;
        if (rplanet) {
            const double rprs = rplanet[w] / rstar;
            r2 = rprs * rprs;
        }
        double v = *out;
        if (f_dilution)
            v *= f_dilution[w];
        v *= r2 / star;
        *out = v;
    }
}

// ---------------------------------------------------------------------------
// Gaussian log-likelihood of band fluxes (pyratbay/tools/retrieval_tools.py:98-104): one
// walker per wavefront, -0.5*sum(((data-model)/uncert)^2) - 0.5*sum(log(2*pi*uncert^2)),
// -inf when not finite.  Sums in lane-strided order, then a fixed butterfly.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_loglike(double *loglike, const double *model,
                                                const double *data, const double *uncert,
                                                int nbands)
{
    const int w = blockIdx.x;
    const double *m = model + (int64_t)w * nbands;
    double chi = 0.0, norm = 0.0;
    for (int b = threadIdx.x; b < nbands; b += 64) {
        const double r = (data[b] - m[b]) / uncert[b];
        chi += r * r;
        norm += log(2.0 * 3.141592653589793 * (uncert[b] * uncert[b]));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        chi += __shfl_xor(chi, d);
        norm += __shfl_xor(norm, d);
    }
    if (threadIdx.x == 0) {
        const double ll = -0.5 * chi - 0.5 * norm;
        loglike[w] = isfinite(ll) ? ll : -1.0e98;     // retrieval_tools.py:101-103
    }
}

// ---------------------------------------------------------------------------
// k_loglike with the data and the uncertainties of each walker
// (Data.offset_data / Data.scale_errors, tools/data.py:210-270, then Loglike.__call__,
// tools/retrieval_tools.py:98-104): one walker per wavefront, sums in lane-strided order, then the
// same butterfly.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_loglike_obs(
    double *loglike, const double *model, const double *data, const double *uncert,
    const int32_t *offset_group, const double *offset_vals, double offset_unit, int noff,
    const int32_t *err_group, const int32_t *err_mode, const double *err_vals, double err_unit,
    int nerr, int nbands)
{
    const int w = blockIdx.x;
    const double *m = model + (int64_t)w * nbands;
    const double *ov = noff ? offset_vals + (int64_t)w * noff : nullptr;
    const double *ev = nerr ? err_vals + (int64_t)w * nerr : nullptr;
    double chi = 0.0, norm = 0.0;
    for (int b = threadIdx.x; b < nbands; b += 64) {
        double d = data[b], u = uncert[b];
        if (ov) {
            const int g = offset_group[b];
            if (g >= 0 && g < noff)
                d = d + ov[g] * offset_unit;
        }
        if (ev) {
            const int g = err_group[b];
            if (g >= 0 && g < nerr) {
                double e = pow(10.0, ev[g]);
                if (err_mode[g] == 0) {
                    u = u * e;
                } else {
                    e *= err_unit;
                    u = sqrt(u * u + e * e);
                }
            }
        }
        const double r = (d - m[b]) / u;
        chi += r * r;
        norm += log(2.0 * 3.141592653589793 * (u * u));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        chi += __shfl_xor(chi, d);
        norm += __shfl_xor(norm, d);
    }
    if (threadIdx.x == 0) {
        const double ll = -0.5 * chi - 0.5 * norm;
        loglike[w] = isfinite(ll) ? ll : -1.0e98;     // retrieval_tools.py:101-103
    }
}

}  // namespace

extern "C" {

int pb_star_band_scale_batch(double *bandflux_d, const double *star_grid_d,
                             const double *sed_temps_d, const double *tstar_d, double rprs2,
                             const double *rplanet_d, double rstar, const double *f_dilution_d,
                             const double *wn_d, const int32_t *band_start_d,
                             const int32_t *band_count_d, const double *response_d,
                             const int64_t *response_offset_d, const double *heights_d, int nt,
                             int nbands, int nwave, int nwalkers, void *stream)
{
    PB_REQUIRE(nbands >= 0 && nwave >= 0 && nwalkers >= 0, "pb_star_band_scale_batch: bad sizes");
    PB_REQUIRE(nt >= 2, "pb_star_band_scale_batch: the grid needs at least 2 temperatures");
    if (nbands == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(bandflux_d && star_grid_d && sed_temps_d && tstar_d && wn_d && band_start_d &&
                   band_count_d && response_d && response_offset_d,
               "pb_star_band_scale_batch: null pointer");
    PB_REQUIRE(!rplanet_d || rstar > 0.0, "pb_star_band_scale_batch: rplanet needs rstar > 0");
    PB_REQUIRE(nwalkers <= 65535, "pb_star_band_scale_batch: at most 65535 walkers per call");
    dim3 grid(nbands, nwalkers);
    k_star_band_scale_batch<<<grid, kBlock, 0, pb::as_stream(stream)>>>(
        bandflux_d, star_grid_d, sed_temps_d, tstar_d, rprs2, rplanet_d, rstar, f_dilution_d, wn_d,
        band_start_d, band_count_d, response_d, response_offset_d, heights_d, nt, nbands, nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_loglike(double *loglike_d, const double *bandflux_d, const double *data_d,
               const double *uncert_d, int nwalkers, int nbands, void *stream)
{
    PB_REQUIRE(nwalkers >= 0 && nbands >= 1, "pb_loglike: bad shape");
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(loglike_d && bandflux_d && data_d && uncert_d, "pb_loglike: null pointer");
    k_loglike<<<nwalkers, 64, 0, pb::as_stream(stream)>>>(loglike_d, bandflux_d, data_d, uncert_d,
                                                         nbands);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_loglike_obs(double *loglike_d, const double *bandflux_d, const double *data_d,
                   const double *uncert_d, const int32_t *offset_group_d,
                   const double *offset_vals_d, double offset_unit, int noff,
                   const int32_t *err_group_d, const int32_t *err_mode_d,
                   const double *err_vals_d, double err_unit, int nerr, int nwalkers, int nbands,
                   void *stream)
{
    PB_REQUIRE(nwalkers >= 0 && nbands >= 1 && noff >= 0 && nerr >= 0,
               "pb_loglike_obs: bad shape");
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(loglike_d && bandflux_d && data_d && uncert_d, "pb_loglike_obs: null pointer");
    PB_REQUIRE(noff == 0 || (offset_group_d && offset_vals_d),
               "pb_loglike_obs: null pointer (offsets)");
    PB_REQUIRE(nerr == 0 || (err_group_d && err_mode_d && err_vals_d),
               "pb_loglike_obs: null pointer (error models)");
    k_loglike_obs<<<nwalkers, 64, 0, pb::as_stream(stream)>>>(
        loglike_d, bandflux_d, data_d, uncert_d, offset_group_d, offset_vals_d, offset_unit, noff,
        err_group_d, err_mode_d, err_vals_d, err_unit, nerr, nbands);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
