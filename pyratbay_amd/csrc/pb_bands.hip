// Band integration, of one spectrum and of a batch of spectra (the last stage of the
// walker-batched retrieval path), the factors applied to band fluxes, and the rejection of walkers
// whose temperatures leave the cross-section table.
#include "pb_common.h"

namespace {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------
// Band integration (PassBand.integrate, pyratbay/spectrum/spec_tools.py:193-233):
// trapezoid over wavenumber of spectrum[idx]*response for each band's contiguous
// index range.  One workgroup per band; only the pairs (i, i+1) whose left sample lies
// in [wbegin, wbegin+wcount) are summed, so that wavenumber shards add up.  The
// per-thread partial sums are combined in a fixed order (reproducible).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_band_integrate(
    double *bandflux, const double *spectrum, const double *wn, const int32_t *band_start,
    const int32_t *band_count, const double *response, const int64_t *response_offset,
    int64_t wbegin, int64_t wcount)
{
    __shared__ double s_part[kBlock];
    const int b = blockIdx.x;
    const int start = band_start[b];
    const int count = band_count[b];
    const double *resp = response + response_offset[b];
    double acc = 0.0;
    for (int i = threadIdx.x; i + 1 < count; i += kBlock) {
        const int64_t g = (int64_t)start + i;
        if (g < wbegin || g >= wbegin + wcount)
            continue;
        const double y0 = spectrum[g] * resp[i];
        const double y1 = spectrum[g + 1] * resp[i + 1];
        acc += 0.5 * (wn[g + 1] - wn[g]) * (y0 + y1);
    }
    s_part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            s_part[threadIdx.x] += s_part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        bandflux[b] = s_part[0];
}

// band fluxes of a batch times a per-walker factor (f_dilution, pyrat_obj.py:296-297: applied to
// the band integral here, to the spectrum in the reference -- the same up to one rounding) and a
// per-band factor (eclipse: rprs^2 / bandflux_star, pyrat_obj.py:662-665), either may be absent
__global__ __launch_bounds__(kBlock) void k_band_scale(double *bandflux, const double *band_scale,
                                                       const double *walker_scale, int nbands,
                                                       int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    double v = bandflux[i];
    if (walker_scale)
        v *= walker_scale[i / nbands];
    if (band_scale)
        v *= band_scale[i % nbands];
    bandflux[i] = v;
}

// ---------------------------------------------------------------------------
// PassBand.integrate for a batch of spectra: grid (band, walker); fixed-order tree sum.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_band_integrate_batch(
    double *bandflux, const double *spectrum, const double *wn, const int32_t *band_start,
    const int32_t *band_count, const double *response, const int64_t *response_offset,
    const double *heights, int nbands, int nwave)
{
    __shared__ double s_part[kBlock];
    const int b = blockIdx.x, w = blockIdx.y;
    const int start = band_start[b];
    const int count = band_count[b];
    const double *resp = response + response_offset[b];
    const double *spec = spectrum + (int64_t)w * nwave;
    double acc = 0.0;
    for (int i = threadIdx.x; i + 1 < count; i += kBlock) {
        const int64_t g = (int64_t)start + i;
        const double y0 = spec[g] * resp[i];
        const double y1 = spec[g + 1] * resp[i + 1];
        acc += 0.5 * (wn[g + 1] - wn[g]) * (y0 + y1);
    }
    s_part[threadIdx.x] = acc;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            s_part[threadIdx.x] += s_part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        bandflux[(int64_t)w * nbands + b] = heights ? s_part[0] * heights[b] : s_part[0];
}

// walkers whose temperatures leave the table: every band flux = +inf (eval()'s reject value,
// pyrat_obj.py:302-320, 378-380)
__global__ __launch_bounds__(kBlock) void k_reject_walkers(double *bandflux, const double *temps,
                                                           double tmin, double tmax, int nlayers,
                                                           int nbands)
{
    __shared__ int s_bad;
    const int w = blockIdx.x;
    if (threadIdx.x == 0)
        s_bad = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < nlayers; k += kBlock) {
        const double t = temps[(int64_t)w * nlayers + k];
        if (!(t >= tmin && t <= tmax))
            s_bad = 1;
    }
    __syncthreads();
    if (s_bad)
        for (int b = threadIdx.x; b < nbands; b += kBlock)
            bandflux[(int64_t)w * nbands + b] = INFINITY;
}

}  // namespace

extern "C" {

int pb_band_integrate(double *bandflux_d, const double *spectrum_d, const double *wn_d,
                      const int32_t *band_start_d, const int32_t *band_count_d,
                      const double *response_d, const int64_t *response_offset_d,
                      int nbands, int64_t wbegin, int64_t wcount, void *stream)
{
    PB_REQUIRE(nbands >= 0 && wbegin >= 0 && wcount >= 0, "pb_band_integrate: bad sizes");
    if (nbands == 0)
        return PB_OK;
    PB_REQUIRE(bandflux_d && spectrum_d && wn_d && band_start_d && band_count_d &&
                   response_d && response_offset_d,
               "pb_band_integrate: null pointer");
    k_band_integrate<<<nbands, kBlock, 0, pb::as_stream(stream)>>>(
        bandflux_d, spectrum_d, wn_d, band_start_d, band_count_d, response_d,
        response_offset_d, wbegin, wcount);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_band_scale(double *bandflux_d, const double *band_scale_d, const double *walker_scale_d,
                  int nbands, int nwalkers, void *stream)
{
    PB_REQUIRE(nbands >= 0 && nwalkers >= 0, "pb_band_scale: bad sizes");
    const int64_t n = (int64_t)nbands * nwalkers;
    if (n == 0 || (!band_scale_d && !walker_scale_d))
        return PB_OK;
    PB_REQUIRE(bandflux_d, "pb_band_scale: null pointer");
    k_band_scale<<<(unsigned)pb::div_up(n, (int64_t)kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        bandflux_d, band_scale_d, walker_scale_d, nbands, n);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_band_integrate_batch(double *bandflux_d, const double *spectrum_d, const double *wn_d,
                            const int32_t *band_start_d, const int32_t *band_count_d,
                            const double *response_d, const int64_t *response_offset_d,
                            const double *heights_d, int nbands, int nwave, int nwalkers,
                            void *stream)
{
    PB_REQUIRE(nbands >= 0 && nwave >= 0 && nwalkers >= 0, "pb_band_integrate_batch: bad sizes");
    if (nbands == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(bandflux_d && spectrum_d && wn_d && band_start_d && band_count_d && response_d &&
                   response_offset_d,
               "pb_band_integrate_batch: null pointer");
    dim3 grid(nbands, nwalkers);
    k_band_integrate_batch<<<grid, kBlock, 0, pb::as_stream(stream)>>>(
        bandflux_d, spectrum_d, wn_d, band_start_d, band_count_d, response_d, response_offset_d,
        heights_d, nbands, nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_reject_walkers(double *bandflux_d, const double *temps_d, double tmin, double tmax,
                      int nlayers, int nbands, int nwalkers, void *stream)
{
    PB_REQUIRE(nlayers >= 1 && nbands >= 0 && nwalkers >= 0, "pb_reject_walkers: bad shape");
    if (nwalkers == 0 || nbands == 0)
        return PB_OK;
    PB_REQUIRE(bandflux_d && temps_d, "pb_reject_walkers: null pointer");
    k_reject_walkers<<<nwalkers, kBlock, 0, pb::as_stream(stream)>>>(bandflux_d, temps_d, tmin,
                                                                   tmax, nlayers, nbands);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
