// Walker-batched retrieval path: band contribution functions (Pyrat.band_contribution,
// pyrat/pyrat_obj.py:671-696 -> spectrum/contribution_funcs.py) per walker, without clouds.
//   k_band_cf_emission     contribution_function + band_cf's integral from ec: the plane-parallel
//                          depth, exp(-depth), B and the per-column normalisation stay in registers
//   k_band_transmittance   transmittance + band_cf's integral from the depth / ideep that
//                          pb_transit_spectrum_batch stores
//   k_band_cf_finish       the bands' parts added in chunk order, divided by their maximum over
//                          the layers
// FP64, no atomics, every sum in a fixed order: two runs give the same bits.
#include "pb_common.h"
#include "pb_planck.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
// LDS of k_band_cf_emission: kT and 1 / kT [2 L], the intervals and d ln p [2 (L - 1)], the
// wavefronts' sums [kWaves L] = (8 L - 2) doubles of the 64 KiB a workgroup gets
constexpr int kMaxLayersEmission = 1024;
// k_band_transmittance keeps only the wavefronts' sums: 4 L doubles
constexpr int kMaxLayersTransit = 2048;

using pb::planck_factor;
using pb::planck_q;
using pb::planck_terms;

// the sum over the wavefront, the same bits in every lane (pb_radeq.hip's)
__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = kWave / 2; off > 0; off >>= 1)
        v += __shfl_xor(v, off, kWave);
    return v;
}

// np.trapezoid as a weight per sample: half of each neighbouring gap INSIDE the band and the grid
// (one-sided at the band's ends and where the grid clips the band, 0 for one retained sample); wn
// is read at g - 1 / g + 1 only inside both, so never outside [0, nwave)
__device__ __forceinline__ double band_weight(const double *wn, int64_t g, int i, int count,
                                              int nwave)
{
    const double x = wn[g];
    double wgt = 0.0;
    if (i > 0 && g > 0)
        wgt += 0.5 * (x - wn[g - 1]);
    if (i + 1 < count && g + 1 < nwave)
        wgt += 0.5 * (wn[g + 1] - x);
    return wgt;
}

// the samples of a band that lie on the grid: [start, start + count) clipped to [0, nwave)
__device__ __forceinline__ int band_retained(int start, int count, int nwave)
{
    const int64_t lo = max(start, 0), hi = min((int64_t)start + count, (int64_t)nwave);
    return (int)max(hi - lo, (int64_t)0);
}

// What the two kernels share: the workgroup's band and chunk, the lane's sample.  The chunks
// count from the band's first sample ON THE GRID, so a clipped band takes the lanes (and with
// them the summation order and the bits) of the in-grid band of its retained samples.
struct Sample {
    int count;        // samples of the band
    int retained;     // those on the grid
    int i;            // this lane's sample within the (unclipped) band
    int64_t g;        // its column on the grid
    bool live;        // inside the band and the grid
};
__device__ __forceinline__ Sample band_sample(const int32_t *band_start, const int32_t *band_count,
                                              int nwave)
{
    Sample s;
    const int b = blockIdx.y;
    const int start = pb::uniform_i32(band_start + b);
    s.count = pb::uniform_i32(band_count + b);
    s.retained = band_retained(start, s.count, nwave);
    const int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x;      // among the retained
    s.live = at < s.retained;
    s.g = max(start, 0) + at;
    s.i = s.live ? (int)(s.g - start) : 0;
    return s;
}

// the four wavefronts' sums of every layer, added in wavefront order -> parts[w][b][chunk][L]
__device__ __forceinline__ void store_parts(double *parts, const double *s_red, int nlayers)
{
    __syncthreads();
    parts += (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * nlayers;
    for (int k = threadIdx.x; k < nlayers; k += kBlock) {
        double v = s_red[k];
        for (int wv = 1; wv < kWaves; wv++)
            v += s_red[wv * nlayers + k];
        parts[k] = v;
    }
}

// ---------------------------------------------------------------------------
// Emission and two-stream geometry.  grid (chunks of 256 samples, bands, walkers); a thread owns a
// column.  Per column (contribution_funcs.py:13-49 on the depth of _trapezoid.c:175-213):
//   depth[k] = 0 for k <= itop and below the stop, the running trapezoid between
//   e[k] = exp(-depth[k]);  detau[k] = e[k+1] - e[k], set to 0 where > 0.1
//   cf[k] = B[k] detau[k] / dlnp[k] (k < L - 1), cf[L-1] = 0;  cf /= sum_k cf
// The first walk gives the column's sum, the second the same values again, divided by it and
// weighted by response x trapezoid weight, summed over the wavefront layer by layer.
// ---------------------------------------------------------------------------
struct EmissionColumn {
    const double *ec;       // this column of the walker's ec: stride nwave
    int64_t nwave;
    double w, factor;
    double acc, prev, eprev;
    bool stopped;

    __device__ __forceinline__ void start(int itop)
    {
        acc = 0.0;
        eprev = 1.0;                                    // exp(-0): rows up to itop
        stopped = false;
        prev = ec[(int64_t)itop * nwave];
    }
    // cf[k] before the normalisation, k = 0 .. L-2 in order
    __device__ __forceinline__ double step(int k, const double *s_kt, const double *s_h,
                                           const double *s_dlp, double maxdepth, int itop,
                                           int ibottom, int nlayers)
    {
        double enext = 1.0;                             // rows up to itop and below the stop: depth 0
        if (k + 1 > itop && !stopped) {
            const double cur = ec[(int64_t)(k + 1) * nwave];
            acc += 0.5 * s_h[k] * (cur + prev);
            prev = cur;
            enext = pb::exp_s(-acc);
            stopped = acc >= maxdepth || k + 1 == ibottom || k + 1 == nlayers - 1;
        }
        double detau = enext - eprev;
        eprev = enext;
        if (detau > 0.1)
            detau = 0.0;                                // the jump back to depth 0 below the stop
        if (detau == 0.0)
            return 0.0;
        return planck_q(factor, w, s_kt[k], s_kt[nlayers + k]) * detau / s_dlp[k];
    }
};

__global__ __launch_bounds__(kBlock) void k_band_cf_emission(
    double *__restrict__ parts, const double *__restrict__ ec, const double *__restrict__ intervals,
    const double *__restrict__ dlogp, const double *__restrict__ wn,
    const double *__restrict__ temps, const int32_t *__restrict__ band_start,
    const int32_t *__restrict__ band_count, const double *__restrict__ response,
    const int64_t *__restrict__ response_offset, double maxdepth, int itop, int ibottom,
    int nlayers, int nwave)
{
    extern __shared__ double s_kt[];                    // [2][L]: kT of this walker, its reciprocal
    const Sample s = band_sample(band_start, band_count, nwave);
    if (blockIdx.x * kBlock >= s.retained)
        return;                                         // (past its last grid sample: uniform)
    double *s_h = s_kt + 2 * nlayers;                   // [L-1]
    double *s_dlp = s_h + (nlayers - 1);                // [L-1]
    double *s_red = s_dlp + (nlayers - 1);              // [kWaves][L]
    const int wk = blockIdx.z;
    for (int k = threadIdx.x; k < nlayers - 1; k += kBlock) {
        s_h[k] = intervals[(int64_t)wk * (nlayers - 1) + k];
        s_dlp[k] = dlogp[k];
    }
    planck_terms(s_kt, temps + (int64_t)wk * nlayers, nlayers);       // (ends with the barrier)

    EmissionColumn c;
    c.nwave = nwave;
    c.ec = ec + (int64_t)wk * nlayers * nwave + (s.live ? s.g : 0);
    c.w = s.live ? wn[s.g] : 1.0;
    c.factor = planck_factor(c.w);
    double *red = s_red + (threadIdx.x / kWave) * nlayers;
    const int lane = threadIdx.x & (kWave - 1);

    // first walk: the column's sum over the layers (np.sum(cf, axis=0): row after row)
    double sum = 0.0;
    if (s.live) {
        c.start(itop);
        for (int k = 0; k < nlayers - 1; k++) {
            sum += c.step(k, s_kt, s_h, s_dlp, maxdepth, itop, ibottom, nlayers);
            // (the rows below: detau = 0 once the jump at the stop has been taken)
            if (c.stopped && c.eprev == 1.0)
                break;
        }
    }
    // second walk: every lane of the wavefront takes every layer (the sums are wave-wide)
    const double scale = s.live ? response[response_offset[blockIdx.y] + s.i] *
                                      band_weight(wn, s.g, s.i, s.count, nwave)
                                : 0.0;
    if (s.live)
        c.start(itop);
    for (int k = 0; k < nlayers - 1; k++) {
        double v = 0.0;
        if (s.live)
            v = c.step(k, s_kt, s_h, s_dlp, maxdepth, itop, ibottom, nlayers) / sum * scale;
        v = wave_sum(v);
        if (lane == 0)
            red[k] = v;
    }
    if (lane == 0)
        red[nlayers - 1] = 0.0;                         // the appended row
    store_parts(parts, s_red, nlayers);
}

// ---------------------------------------------------------------------------
// Transit geometry (contribution_funcs.py:52-71): exp(-depth[r]) for r < ideep, 0 from row ideep
// on.  The rows above itop have depth 0 in the reference: transmittance 1, not read here.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_band_transmittance(
    double *__restrict__ parts, const double *__restrict__ depth,
    const int32_t *__restrict__ ideep, const double *__restrict__ wn,
    const int32_t *__restrict__ band_start, const int32_t *__restrict__ band_count,
    const double *__restrict__ response, const int64_t *__restrict__ response_offset, int itop,
    int nlayers, int nwave)
{
    extern __shared__ double s_red[];                   // [kWaves][L]
    const Sample s = band_sample(band_start, band_count, nwave);
    if (blockIdx.x * kBlock >= s.retained)
        return;
    const int wk = blockIdx.z;
    const double *col = depth + (int64_t)wk * nlayers * nwave + (s.live ? s.g : 0);
    int deep = 0;
    double scale = 0.0;
    if (s.live) {
        deep = min(max(ideep[(int64_t)wk * nwave + s.g], 0), nlayers);
        scale = response[response_offset[blockIdx.y] + s.i] * band_weight(wn, s.g, s.i, s.count,
                                                                         nwave);
    }
    double *red = s_red + (threadIdx.x / kWave) * nlayers;
    const int lane = threadIdx.x & (kWave - 1);
    for (int r = 0; r < nlayers; r++) {
        double v = 0.0;
        if (r < deep) {
            const double t = r < itop ? 1.0 : pb::exp_s(-col[(int64_t)r * nwave]);
            v = t * scale;
        }
        v = wave_sum(v);
        if (lane == 0)
            red[r] = v;
    }
    store_parts(parts, s_red, nlayers);
}

// ---------------------------------------------------------------------------
// band_cf's normalisation: grid (bands, walkers).  The band's chunks are added in chunk order, the
// maximum over the layers is np.amax's (a NaN anywhere gives NaN), and every layer is divided by
// it: a band of one sample (or none) is 0 / 0 = NaN in every layer, as in the reference.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double nan_max(double a, double b)
{
    return (a != a) ? a : (b != b) ? b : (a > b ? a : b);
}

__global__ __launch_bounds__(kBlock) void k_band_cf_finish(double *__restrict__ out,
                                                           const double *__restrict__ parts,
                                                           const int32_t *__restrict__ band_start,
                                                           const int32_t *__restrict__ band_count,
                                                           int nbands, int nchunks, int nlayers,
                                                           int nwave)
{
    __shared__ double s_max[kBlock];
    const int b = blockIdx.x, wk = blockIdx.y;
    const int retained = band_retained(pb::uniform_i32(band_start + b),
                                       pb::uniform_i32(band_count + b), nwave);
    // (the chunks past the band's last sample on the grid were never written)
    const int used = (int)min(((int64_t)retained + kBlock - 1) / kBlock, (int64_t)nchunks);
    parts += ((int64_t)wk * nbands + b) * nchunks * nlayers;
    double m = -INFINITY;
    for (int k = threadIdx.x; k < nlayers; k += kBlock) {
        double v = 0.0;
        for (int c = 0; c < used; c++)
            v += parts[(int64_t)c * nlayers + k];
        m = nan_max(m, v);
    }
    s_max[threadIdx.x] = m;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            s_max[threadIdx.x] = nan_max(s_max[threadIdx.x], s_max[threadIdx.x + h]);
        __syncthreads();
    }
    m = s_max[0];
    for (int k = threadIdx.x; k < nlayers; k += kBlock) {
        double v = 0.0;
        for (int c = 0; c < used; c++)
            v += parts[(int64_t)c * nlayers + k];
        out[((int64_t)wk * nlayers + k) * nbands + b] = v / m;
    }
}

int finish(double *out_d, const double *work_d, const int32_t *band_start_d,
           const int32_t *band_count_d, int nbands, int nchunks, int nlayers, int nwave,
           int nwalkers, void *stream)
{
    k_band_cf_finish<<<dim3(nbands, nwalkers), kBlock, 0, pb::as_stream(stream)>>>(
        out_d, work_d, band_start_d, band_count_d, nbands, nchunks, nlayers, nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace

extern "C" {

int64_t pb_band_contribution_work_doubles(int nlayers, int nbands, int max_band_count,
                                          int nwalkers)
{
    if (nlayers < 1 || nbands < 1 || max_band_count < 1 || nwalkers < 1)
        return 0;
    return (int64_t)nwalkers * nbands * pb::div_up(max_band_count, kBlock) * nlayers;
}

int pb_band_contribution_emission_batch(double *out_d, const double *ec_d,
                                        const double *intervals_d, const double *dlogp_d,
                                        const double *wn_d, const double *temps_d,
                                        const int32_t *band_start_d, const int32_t *band_count_d,
                                        const double *response_d,
                                        const int64_t *response_offset_d, int max_band_count,
                                        double maxdepth, int itop, int ibottom, int nlayers,
                                        int nwave, int nbands, int nwalkers, double *work_d,
                                        void *stream)
{
    PB_REQUIRE(nlayers >= 2 && nwave >= 1 && nbands >= 0 && nwalkers >= 0 && max_band_count >= 0,
               "pb_band_contribution_emission_batch: bad sizes (nlayers >= 2, nwave >= 1)");
    PB_REQUIRE(nlayers <= kMaxLayersEmission,
               "pb_band_contribution_emission_batch: %d layers, at most %d fit in the LDS of a "
               "workgroup", nlayers, kMaxLayersEmission);
    PB_REQUIRE(itop >= 0 && itop < nlayers, "pb_band_contribution_emission_batch: itop out of range");
    PB_REQUIRE(ibottom <= nlayers, "pb_band_contribution_emission_batch: ibottom > nlayers");
    PB_REQUIRE(nbands <= 65535 && nwalkers <= 65535,
               "pb_band_contribution_emission_batch: at most 65535 bands and walkers per call");
    if (nbands == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(out_d && ec_d && intervals_d && dlogp_d && wn_d && temps_d && band_start_d &&
                   band_count_d && response_d && response_offset_d,
               "pb_band_contribution_emission_batch: null pointer");
    const int nchunks = pb::div_up(max_band_count, kBlock);
    PB_REQUIRE(nchunks == 0 || work_d, "pb_band_contribution_emission_batch: null work buffer");
    if (nchunks > 0) {
        const size_t lds = ((size_t)(4 + kWaves) * nlayers - 2) * sizeof(double);
        k_band_cf_emission<<<dim3(nchunks, nbands, nwalkers), kBlock, lds, pb::as_stream(stream)>>>(
            work_d, ec_d, intervals_d, dlogp_d, wn_d, temps_d, band_start_d, band_count_d,
            response_d, response_offset_d, maxdepth, itop, ibottom, nlayers, nwave);
        PB_LAUNCH_CHECK();
    }
    return finish(out_d, work_d, band_start_d, band_count_d, nbands, nchunks, nlayers, nwave,
                  nwalkers, stream);
}

int pb_band_transmittance_batch(double *out_d, const double *depth_d, const int32_t *ideep_d,
                                const double *wn_d, const int32_t *band_start_d,
                                const int32_t *band_count_d, const double *response_d,
                                const int64_t *response_offset_d, int max_band_count, int itop,
                                int nlayers, int nwave, int nbands, int nwalkers, double *work_d,
                                void *stream)
{
    PB_REQUIRE(nlayers >= 1 && nwave >= 1 && nbands >= 0 && nwalkers >= 0 && max_band_count >= 0,
               "pb_band_transmittance_batch: bad sizes");
    PB_REQUIRE(nlayers <= kMaxLayersTransit,
               "pb_band_transmittance_batch: %d layers, at most %d fit in the LDS of a workgroup",
               nlayers, kMaxLayersTransit);
    PB_REQUIRE(itop >= 0 && itop < nlayers, "pb_band_transmittance_batch: itop out of range");
    PB_REQUIRE(nbands <= 65535 && nwalkers <= 65535,
               "pb_band_transmittance_batch: at most 65535 bands and walkers per call");
    if (nbands == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(out_d && depth_d && ideep_d && wn_d && band_start_d && band_count_d && response_d &&
                   response_offset_d,
               "pb_band_transmittance_batch: null pointer");
    const int nchunks = pb::div_up(max_band_count, kBlock);
    PB_REQUIRE(nchunks == 0 || work_d, "pb_band_transmittance_batch: null work buffer");
    if (nchunks > 0) {
        const size_t lds = (size_t)kWaves * nlayers * sizeof(double);
        k_band_transmittance<<<dim3(nchunks, nbands, nwalkers), kBlock, lds,
                               pb::as_stream(stream)>>>(
            work_d, depth_d, ideep_d, wn_d, band_start_d, band_count_d, response_d,
            response_offset_d, itop, nlayers, nwave);
        PB_LAUNCH_CHECK();
    }
    return finish(out_d, work_d, band_start_d, band_count_d, nbands, nchunks, nlayers, nwave,
                  nwalkers, stream);
}

}  // extern "C"
