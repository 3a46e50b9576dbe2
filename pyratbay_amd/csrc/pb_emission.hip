// Emission geometry: plane-parallel optical depth, Planck function, intensity per angle and the
// quadrature over angles -- as separate passes for one spectrum and as ONE pass for a batch of
// walkers (k_emission_fused, the retrieval inner loop).  A thread owns a column: the
// [layer][wavenumber] arrays are row-major so that the 64 lanes of a wavefront read 512 contiguous
// bytes of one layer and walk down the layers; per-layer scalars (intervals, temperatures, mu) are
// wave-uniform and come through the scalar cache or LDS.
//
// Reference functions restated (pyratbay v2.0.1): src_c/_trapezoid.c:175-213 and 304-341,
// src_c/_blackbody.c:35-130 and the Python loop pyratbay/pyrat/spectrum.py:366-377.
#include "pb_common.h"
#include "pb_planck.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxMu = 16;

// ---------------------------------------------------------------------------
// What the reference makes of a plane-parallel flux AFTER the radiative transfer, per sample
// (pyrat/spectrum.py:394-405 and eval()'s unit conversion, pyrat_obj.py:323-329):
//   fplanet  = flux [* f_dilution]
//   emission : spectrum = fplanet
//   eclipse  : spectrum = fplanet * (1/starflux * rprs2),     rprs2 = (rplanet/rstar)^2
//   f_lambda : spectrum = 10.0 * fplanet * (rd * wn * 1e-4)^2, rd = rplanet/distance
// Same products in the same order as the NumPy expressions (bit-equal); `scale` is rprs2 or rd.
// spectrum and fplanet may alias flux (the reference's `spec.fplanet = spec.spectrum`).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_emission_observables(
    double *spectrum, double *fplanet, const double *flux, const double *starflux,
    const double *wn, int64_t n, int mode, int dilute, double f_dilution, double scale)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    double f = flux[i];
    if (dilute)
        f *= f_dilution;
    double s = f;
    if (mode == 1) {
        const double fstar_rprs = 1.0 / starflux[i] * scale;
        s = f * fstar_rprs;
    } else if (mode == 2) {
        const double t = scale * wn[i] * 1.0e-4;
        s = 10.0 * f * (t * t);
    }
    if (fplanet)
        fplanet[i] = f;
    spectrum[i] = s;
}

// ---------------------------------------------------------------------------
// _trapezoid.plane_parallel_optical_depth (src_c/_trapezoid.c:175-213)
// ---------------------------------------------------------------------------
__global__ void k_plane_depth(double *depth, int32_t *ideep, const double *ec,
                              const double *h, double maxdepth, int itop, int ibottom,
                              int nlayers, int nwave)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwave)
        return;
    double acc = 0.0;
    for (int k = 0; k <= itop && k < nlayers; k++)
        depth[(int64_t)k * nwave + i] = 0.0;
    double prev = itop < nlayers ? ec[(int64_t)itop * nwave + i] : 0.0;
    // The rows are fetched eight at a time and then examined in order: with the stop rule
    // inside a one-row loop every load waited for the previous row's branch (64 us for 128 MB
    // at 1e5 samples: 80 exposed latencies per column).  Rows past the stop are loaded (inside
    // the array) and dropped; the sums and the stop are the reference's.
    constexpr int kFetch = 8;
    int k = min(itop, nlayers - 1), stop = -1;
    for (int k0 = itop + 1; k0 < nlayers && stop < 0; k0 += kFetch) {
        double cur[kFetch];
#pragma unroll
        for (int q = 0; q < kFetch; q++)
            cur[q] = ec[(int64_t)min(k0 + q, nlayers - 1) * nwave + i];
#pragma unroll
        for (int q = 0; q < kFetch; q++) {
            if (stop >= 0 || k0 + q >= nlayers)
                continue;
            k = k0 + q;
            acc += 0.5 * h[k - 1] * (cur[q] + prev);
            prev = cur[q];
            depth[(int64_t)k * nwave + i] = acc;
            if (acc >= maxdepth || k == ibottom || k == nlayers - 1)
                stop = k;
        }
    }
    // (the one-row loop ended with k == nlayers when no row was examined after itop)
    ideep[i] = stop >= 0 ? stop : (itop + 1 >= nlayers ? nlayers : k);
}

// ---------------------------------------------------------------------------
// Planck function (src_c/_blackbody.c:35-130)
// ---------------------------------------------------------------------------
// (pb_planck.h: shared with pb_two_stream.hip and pb_clouds.hip)
using pb::planck;
using pb::planck_factor;
using pb::planck_q;
using pb::planck_terms;

__global__ void k_blackbody2d(double *B, const double *wn, int nwave, const double *temp,
                              int nlayers, const int32_t *last)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int j = blockIdx.y;
    if (i >= nwave)
        return;
    int ilast = last ? last[i] : nlayers - 1;
    if (j > ilast)
        return;
    double w = wn[i];
    B[(int64_t)j * nwave + i] = planck(planck_factor(w), w, temp[j]);
}

__global__ void k_blackbody1d(double *B, const double *wn, int nwave, double temp)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwave)
        return;
    double w = wn[i];
    B[i] = planck(planck_factor(w), w, temp);
}

// ---------------------------------------------------------------------------
// _trapezoid.intensity (src_c/_trapezoid.c:304-341; tdiff/itrapezoid utils.h:6-41)
// one thread per (column, mu)
// ---------------------------------------------------------------------------
__global__ void k_intensity(double *out, const double *tau, const int32_t *ideep,
                            const double *bbody, const double *mu, int nmu, int rtop,
                            int nlayers, int nwave)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    int k = blockIdx.y;
    if (j >= nwave)
        return;
    int last = ideep[j];
    if (last > nlayers - 1)
        last = nlayers - 1;
    double m, im;
    pb::sane_divisor(mu[k], m, im);
    double blast = bbody[(int64_t)last * nwave + j];
    double result;
    if (last - rtop == 1) {
        result = blast;
    } else {
        double acc = 0.0;
        if (last > rtop) {
            double eprev = pb::exp_s(pb::quot_fast(-pb::clamp_depth(tau[(int64_t)rtop * nwave + j]), m, im));
            double bprev = bbody[(int64_t)rtop * nwave + j];
            for (int i = rtop; i < last; i++) {
                double enext = pb::exp_s(pb::quot_fast(-pb::clamp_depth(tau[(int64_t)(i + 1) * nwave + j]), m, im));
                double bnext = bbody[(int64_t)(i + 1) * nwave + j];
                acc += (enext - eprev) * (bnext + bprev);
                eprev = enext;
                bprev = bnext;
            }
        }
        result = blast * pb::exp_s(pb::quot_fast(-pb::clamp_depth(tau[(int64_t)last * nwave + j]), m, im)) - 0.5 * acc;
    }
    out[(int64_t)k * nwave + j] = result;
}

// ---------------------------------------------------------------------------
// Fused emission: Planck in registers + intensity for every mu + quadrature sum
// (pyrat/spectrum.py:366-377).  One thread per column, layers outermost so that
// tau is read once; the nmu running sums live in registers.
// ---------------------------------------------------------------------------
template <int MU>
__global__ void k_emission_flux(double *flux, double *intensity, const double *tau,
                                const int32_t *ideep, const double *wn,
                                const double *temp, const double *mu,
                                const double *weights, int nmu, int rtop, int nlayers,
                                int nwave, int ideep_max)
{
    extern __shared__ double s_kt[];        // [2][nlayers]: kKB T and its reciprocal
    planck_terms(s_kt, temp, nlayers, mu, nmu);
    const double *s_imu = s_kt + 2 * nlayers;
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nwave)
        return;
    int last = min(ideep[j], ideep_max);    // np.clip(ideep, 0, cloud_itop) with a cloud deck
    if (last > nlayers - 1)
        last = nlayers - 1;
    const double w = wn[j];
    const double factor = planck_factor(w);
    double acc[MU], eprev[MU];
    double t0 = pb::clamp_depth(tau[(int64_t)rtop * nwave + j]);
#pragma unroll
    for (int k = 0; k < MU; k++) {
        acc[k] = 0.0;
        eprev[k] = k < nmu ? pb::exp_s(pb::quot_fast(-t0, mu[k], s_imu[k])) : 0.0;
    }
    double bprev = planck_q(factor, w, s_kt[rtop], s_kt[nlayers + rtop]);
    double tlast = t0;
    for (int i = rtop; i < last; i++) {
        double t = pb::clamp_depth(tau[(int64_t)(i + 1) * nwave + j]);
        double bnext = planck_q(factor, w, s_kt[i + 1], s_kt[nlayers + i + 1]);
        double bsum = bnext + bprev;
#pragma unroll
        for (int k = 0; k < MU; k++) {
            if (k < nmu) {
                double enext = pb::exp_s(pb::quot_fast(-t, mu[k], s_imu[k]));
                acc[k] += (enext - eprev[k]) * bsum;
                eprev[k] = enext;
            }
        }
        bprev = bnext;
        tlast = t;
    }
    double blast = (last > rtop) ? bprev : planck_q(factor, w, s_kt[last], s_kt[nlayers + last]);
    if (last <= rtop)
        tlast = pb::clamp_depth(tau[(int64_t)last * nwave + j]);
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < MU; k++) {
        if (k < nmu) {
            double val;
            if (last - rtop == 1)
                val = blast;
            else
                val = blast * pb::exp_s(pb::quot_fast(-tlast, mu[k], s_imu[k])) - 0.5 * acc[k];
            if (intensity)
                intensity[(int64_t)k * nwave + j] = val;
            total += val * weights[k];
        }
    }
    flux[j] = total;
}

// ---------------------------------------------------------------------------
// Plane-parallel optical depth + emission flux in ONE pass, for a batch of walkers (the
// retrieval inner loop in emission geometry): the running optical depth of k_plane_depth
// (_trapezoid.c:175-213) feeds the intensity sums of k_emission_flux (_trapezoid.c:304-341 +
// pyrat/spectrum.py:366-377) layer by layer, so depth is neither written nor read.  Same
// operations in the same order as the two kernels run one after the other.
// grid (columns, walkers); ec[nw][L][W], intervals[nw][L-1], temp[nw][L] -> flux[nw][W].
// ---------------------------------------------------------------------------
template <int MU>
__global__ void k_emission_fused(double *flux, const double *ec, const double *intervals,
                                 const double *wn, const double *temp, const double *mu,
                                 const double *weights, int nmu, double maxdepth, int itop,
                                 int ibottom, int nlayers, int nwave, const int32_t *scatter,
                                 pb::TileLimit lim, int32_t *flags)
{
    extern __shared__ double s_kt[];        // [2][nlayers]: kKB T of this walker and its reciprocal
    const int wk = blockIdx.y;
    if (lim.gate && pb::uniform_i32(lim.gate + wk) == 0)
        return;                             // (repair pass: walker wk was not flagged)
    planck_terms(s_kt, temp + (int64_t)wk * nlayers, nlayers, mu, nmu);
    const double *s_imu = s_kt + 2 * nlayers;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nwave)
        return;
    ec += (int64_t)wk * nlayers * nwave;
    const double *h = intervals + (int64_t)wk * (nlayers - 1);
    const double w = wn[j];
    const double factor = planck_factor(w);
    const int rtop = itop;
    double acc[MU], eprev[MU];
#pragma unroll
    for (int k = 0; k < MU; k++) {
        acc[k] = 0.0;
        eprev[k] = k < nmu ? pb::exp_s(pb::quot_fast(-0.0, mu[k], s_imu[k])) : 0.0;   // depth[rtop] = 0
    }
    double bprev = planck_q(factor, w, s_kt[rtop], s_kt[nlayers + rtop]);
    double depth = 0.0, tlast = 0.0;
    double prev = ec[(int64_t)itop * nwave + j];
    int last = rtop;                                          // deepest layer seen so far
    // the last layer that was interpolated for this block of 256 (ordered) columns (TileLimit:
    // workgroups are 256 columns wide, so the limit is uniform); a column still open beyond it
    // goes to the repair pass
    const int klim = lim.tile ? lim.row0 + 16 * (pb::uniform_i32(lim.tile + blockIdx.x) + 1) - 1
                              : nlayers;
    bool overrun = false;
    for (int k = itop + 1; k < nlayers; k++) {
        if (k > klim) {
            overrun = true;
            break;
        }
        const double cur = ec[(int64_t)k * nwave + j];
        depth += 0.5 * h[k - 1] * (cur + prev);
        prev = cur;
        // intensity terms of the interval (k-1, k)
        const double bnext = planck_q(factor, w, s_kt[k], s_kt[nlayers + k]);
        const double bsum = bnext + bprev;
        const double dq = pb::clamp_depth(depth);             // (exp(-inf / mu) = 0 without a NaN)
#pragma unroll
        for (int m = 0; m < MU; m++) {
            if (m < nmu) {
                const double enext = pb::exp_s(pb::quot_fast(-dq, mu[m], s_imu[m]));
                acc[m] += (enext - eprev[m]) * bsum;
                eprev[m] = enext;
            }
        }
        bprev = bnext;
        tlast = depth;
        last = k;
        if (depth >= maxdepth || k == ibottom || k == nlayers - 1)
            break;
    }
    if (overrun) {
        if (flags) {
            flags[wk] = 1;
            flags[gridDim.y] = 1;                             // flags[nwalkers]: any walker
        }
        return;                                               // (the repair pass writes this column)
    }
    // (itop == nlayers-1: no interval; the reference's loop then leaves ideep = nlayers, clipped)
    const double blast =
        (last > rtop) ? bprev : planck_q(factor, w, s_kt[last], s_kt[nlayers + last]);
    double total = 0.0;
#pragma unroll
    for (int m = 0; m < MU; m++) {
        if (m < nmu) {
            double val;
            if (last - rtop == 1)
                val = blast;
            else
                val = blast * pb::exp_s(pb::quot_fast(-pb::clamp_depth(tlast), mu[m], s_imu[m])) - 0.5 * acc[m];
            total += val * weights[m];
        }
    }
    // (ordered batches: column j of ec / wn is column scatter[j] of the grid; an index outside
    // the grid is dropped, not written out of bounds)
    const int dst = scatter ? scatter[j] : j;
    if (dst >= 0 && dst < nwave)
        flux[(int64_t)wk * nwave + dst] = total;
}

// the walker batch behind pb_emission_flux_batch / _ordered / _limited
int emission_batch(double *flux_d, const double *ec_d, const double *intervals_d,
                   const double *wn_d, const double *temp_d, const double *mu_d,
                   const double *weights_d, const int32_t *column_d, int nmu, double maxdepth,
                   int itop, int ibottom, int nlayers, int nwave, int nwalkers, void *stream,
                   const int32_t *tile_limit_d = nullptr, int32_t *flags_d = nullptr,
                   const int32_t *gate_d = nullptr)
{
    const pb::TileLimit lim{tile_limit_d, itop, gate_d};
    PB_REQUIRE(nlayers >= 1 && nwave >= 0 && nwalkers >= 0, "pb_emission_flux_batch: bad shape");
    PB_REQUIRE(nmu >= 1 && nmu <= kMaxMu, "pb_emission_flux_batch: nmu must be 1..%d", kMaxMu);
    PB_REQUIRE(itop >= 0 && itop < nlayers, "pb_emission_flux_batch: itop out of range");
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(flux_d && ec_d && wn_d && temp_d && mu_d && weights_d &&
                   (nlayers == 1 || intervals_d),
               "pb_emission_flux_batch: null pointer");
    dim3 grid(pb::div_up(nwave, kBlock), nwalkers);
    // (quadratures of up to 8 angles -- the default raygrid has 5 -- keep 2 x 8 running values per
    // lane instead of 2 x 16: half the registers, twice the wavefronts per SIMD)
    if (nmu <= 8)
        k_emission_fused<8><<<grid, kBlock, ((size_t)2 * nlayers + kMaxMu) * 8, pb::as_stream(stream)>>>(
        flux_d, ec_d, intervals_d, wn_d, temp_d, mu_d, weights_d, nmu, maxdepth, itop, ibottom,
        nlayers, nwave, column_d, lim, flags_d);
    else
        k_emission_fused<kMaxMu><<<grid, kBlock, ((size_t)2 * nlayers + kMaxMu) * 8, pb::as_stream(stream)>>>(
        flux_d, ec_d, intervals_d, wn_d, temp_d, mu_d, weights_d, nmu, maxdepth, itop, ibottom,
        nlayers, nwave, column_d, lim, flags_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int pb_plane_parallel_optical_depth(double *depth_d, int32_t *ideep_d,
                                    const double *ec_d, const double *intervals_d,
                                    double maxdepth, int itop, int ibottom, int nlayers,
                                    int nwave, void *stream)
{
    PB_REQUIRE(nlayers > 0 && nwave >= 0, "pb_plane_parallel_optical_depth: bad shape");
    PB_REQUIRE(itop >= 0, "pb_plane_parallel_optical_depth: itop < 0");
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(depth_d && ideep_d && ec_d && (nlayers == 1 || intervals_d),
               "pb_plane_parallel_optical_depth: null pointer");
    k_plane_depth<<<pb::div_up(nwave, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        depth_d, ideep_d, ec_d, intervals_d, maxdepth, itop, ibottom, nlayers, nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_blackbody_wn_2D(double *B_d, const double *wn_d, int nwave, const double *temp_d,
                       int nlayers, const int32_t *last_d, void *stream)
{
    PB_REQUIRE(nwave >= 0 && nlayers >= 0, "pb_blackbody_wn_2D: bad shape");
    if (nwave == 0 || nlayers == 0)
        return PB_OK;
    PB_REQUIRE(B_d && wn_d && temp_d, "pb_blackbody_wn_2D: null pointer");
    PB_REQUIRE(nlayers <= 65535, "pb_blackbody_wn_2D: too many layers");
    dim3 grid(pb::div_up(nwave, kBlock), nlayers);
    k_blackbody2d<<<grid, kBlock, 0, pb::as_stream(stream)>>>(B_d, wn_d, nwave, temp_d,
                                                            nlayers, last_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_blackbody_wn(double *B_d, const double *wn_d, int nwave, double temp, void *stream)
{
    PB_REQUIRE(nwave >= 0, "pb_blackbody_wn: bad shape");
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(B_d && wn_d, "pb_blackbody_wn: null pointer");
    k_blackbody1d<<<pb::div_up(nwave, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        B_d, wn_d, nwave, temp);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_emission_observables(double *spectrum_d, double *fplanet_d, const double *flux_d,
                            const double *starflux_d, const double *wn_d, int64_t nwave, int mode,
                            int dilute, double f_dilution, double scale, void *stream)
{
    PB_REQUIRE(nwave >= 0, "pb_emission_observables: bad shape");
    PB_REQUIRE(mode >= 0 && mode <= 2, "pb_emission_observables: mode %d (0 emission, 1 eclipse, "
                                      "2 f_lambda)", mode);
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(spectrum_d && flux_d, "pb_emission_observables: null pointer");
    PB_REQUIRE(mode != 1 || starflux_d, "pb_emission_observables: eclipse needs the stellar flux");
    PB_REQUIRE(mode != 2 || wn_d, "pb_emission_observables: f_lambda needs the wavenumbers");
    k_emission_observables<<<(unsigned)pb::div_up(nwave, (int64_t)kBlock), kBlock, 0,
                             pb::as_stream(stream)>>>(spectrum_d, fplanet_d, flux_d, starflux_d,
                                                      wn_d, nwave, mode, dilute, f_dilution, scale);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_intensity(double *out_d, const double *tau_d, const int32_t *ideep_d,
                 const double *bbody_d, const double *mu_d, int nmu, int rtop,
                 int nlayers, int nwave, void *stream)
{
    PB_REQUIRE(nlayers > 0 && nwave >= 0 && nmu >= 0, "pb_intensity: bad shape");
    PB_REQUIRE(rtop >= 0 && rtop < nlayers, "pb_intensity: rtop out of range");
    if (nwave == 0 || nmu == 0)
        return PB_OK;
    PB_REQUIRE(out_d && tau_d && ideep_d && bbody_d && mu_d, "pb_intensity: null pointer");
    dim3 grid(pb::div_up(nwave, kBlock), nmu);
    k_intensity<<<grid, kBlock, 0, pb::as_stream(stream)>>>(out_d, tau_d, ideep_d, bbody_d,
                                                          mu_d, nmu, rtop, nlayers, nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_emission_flux(double *flux_d, double *intensity_d, const double *tau_d,
                     const int32_t *ideep_d, const double *wn_d, const double *temp_d,
                     const double *mu_d, const double *weights_d, int nmu, int rtop,
                     int nlayers, int nwave, void *stream)
{
    return pb_emission_flux_deck(flux_d, intensity_d, tau_d, ideep_d, wn_d, temp_d, mu_d,
                                 weights_d, nmu, rtop, -1, nlayers, nwave, stream);
}

int pb_emission_flux_deck(double *flux_d, double *intensity_d, const double *tau_d,
                          const int32_t *ideep_d, const double *wn_d, const double *temp_d,
                          const double *mu_d, const double *weights_d, int nmu, int rtop,
                          int cloud_itop, int nlayers, int nwave, void *stream)
{
    PB_REQUIRE(nlayers > 0 && nwave >= 0, "pb_emission_flux: bad shape");
    PB_REQUIRE(cloud_itop < nlayers, "pb_emission_flux: cloud_itop out of range");
    PB_REQUIRE(nmu >= 1 && nmu <= kMaxMu, "pb_emission_flux: nmu must be in [1,%d]", kMaxMu);
    PB_REQUIRE(rtop >= 0 && rtop < nlayers, "pb_emission_flux: rtop out of range");
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(flux_d && tau_d && ideep_d && wn_d && temp_d && mu_d && weights_d,
               "pb_emission_flux: null pointer");
    if (nmu <= 8)
        k_emission_flux<8><<<pb::div_up(nwave, kBlock), kBlock, ((size_t)2 * nlayers + kMaxMu) * 8, pb::as_stream(stream)>>>(
        flux_d, intensity_d, tau_d, ideep_d, wn_d, temp_d, mu_d, weights_d, nmu, rtop,
        nlayers, nwave, cloud_itop >= 0 ? cloud_itop : nlayers - 1);
    else
        k_emission_flux<kMaxMu><<<pb::div_up(nwave, kBlock), kBlock, ((size_t)2 * nlayers + kMaxMu) * 8, pb::as_stream(stream)>>>(
        flux_d, intensity_d, tau_d, ideep_d, wn_d, temp_d, mu_d, weights_d, nmu, rtop,
        nlayers, nwave, cloud_itop >= 0 ? cloud_itop : nlayers - 1);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_emission_flux_batch(double *flux_d, const double *ec_d, const double *intervals_d,
                           const double *wn_d, const double *temp_d, const double *mu_d,
                           const double *weights_d, int nmu, double maxdepth, int itop,
                           int ibottom, int nlayers, int nwave, int nwalkers, void *stream)
{
    return emission_batch(flux_d, ec_d, intervals_d, wn_d, temp_d, mu_d, weights_d, nullptr, nmu,
                          maxdepth, itop, ibottom, nlayers, nwave, nwalkers, stream);
}

int pb_emission_flux_ordered(double *flux_d, const double *ec_d, const double *intervals_d,
                             const double *wn_d, const double *temp_d, const double *mu_d,
                             const double *weights_d, const int32_t *column_d, int nmu,
                             double maxdepth, int itop, int ibottom, int nlayers, int nwave,
                             int nwalkers, void *stream)
{
    PB_REQUIRE(column_d || nwave == 0, "pb_emission_flux_ordered: null column index");
    return emission_batch(flux_d, ec_d, intervals_d, wn_d, temp_d, mu_d, weights_d, column_d, nmu,
                          maxdepth, itop, ibottom, nlayers, nwave, nwalkers, stream);
}

int pb_emission_flux_limited(double *flux_d, const double *ec_d, const double *intervals_d,
                             const double *wn_d, const double *temp_d, const double *mu_d,
                             const double *weights_d, const int32_t *column_d, int nmu,
                             double maxdepth, int itop, int ibottom, int nlayers, int nwave,
                             int nwalkers, const int32_t *tile_limit_d, int32_t *flags_d,
                             const int32_t *gate_d, void *stream)
{
    PB_REQUIRE(column_d || nwave == 0, "pb_emission_flux_limited: null column index");
    PB_REQUIRE(!tile_limit_d || flags_d,
               "pb_emission_flux_limited: a tile limit needs flags[nwalkers + 1] to report the "
               "walkers that ran past it");
    return emission_batch(flux_d, ec_d, intervals_d, wn_d, temp_d, mu_d, weights_d, column_d, nmu,
                          maxdepth, itop, ibottom, nlayers, nwave, nwalkers, stream, tile_limit_d,
                          flags_d, gate_d);
}

}  // extern "C"
