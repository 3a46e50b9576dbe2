// Walker-batched retrieval path: band contribution functions (Pyrat.band_contribution,
// pyrat/pyrat_obj.py:671-696 -> spectrum/contribution_funcs.py) per walker, clear and with clouds
// (an opaque deck, cloud-type opacity ec_cloud, a patchy fraction).
//   k_band_cf_emission     contribution_function + band_cf's integral from ec: the plane-parallel
//                          depth, exp(-depth), B and the per-column normalisation stay in registers
//   k_band_transmittance   transmittance + band_cf's integral from the depth / ideep that
//                          pb_transit_spectrum_batch stores
//   k_band_cf_finish       the bands' parts added in chunk order, divided by their maximum over
//                          the layers
// With clouds (the reference's rules are written out at the kernels):
//   k_band_cf_emission<true>      the same two walks on ec + ec_cloud down to the walker's deck,
//                                 whose temperature takes the deck layer's place in B
//   k_band_transmittance_cloudy   transmittance of the clear and the cloudy column + band_cf's
//                                 integral FROM ec, no depth stored for either column
// The cloudy column, the patchy mix and the transit walk over blocks of impact parameters are the
// flux kernels' (pb_clouds.hip): both take them from pb_cloud_walk.h.
// FP64, no atomics, every sum in a fixed order: two runs give the same bits.
#include "pb_cloud_walk.h"
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
// k_band_transmittance_cloudy: the wavefronts' sums and the ray-path segments of a block of
// kCloudyRows impact parameters, (4 L + kCloudyRows (L - itop)) doubles
constexpr int kCloudyRows = 16;
constexpr int kMaxLayersCloudyTransit = PB_BAND_CLOUDY_MAX_LAYERS;
static_assert((size_t)(kWaves + kCloudyRows) * kMaxLayersCloudyTransit * sizeof(double) <=
                  64 * 1024, "the cloudy transmittance kernel's LDS");

using pb::planck_factor;
using pb::planck_q;
using pb::planck_terms;

using pb::CloudWalk;
using pb::uniform_f64;
using pb::wave_sum;

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
// kCloudy (pyrat_obj.py:135-139, 691-693; spectrum/radiative_transfer.py:125-127): the column is
// ec + ec_cloud, ibottom = deck_itop[walker] + 1 -- the reference's loop stores row ibottom before
// it stops, so the depth runs through the row past the deck -- and the deck's temperature takes
// the place of the layer's in row deck_itop of B.  The cloudy column ONLY, patchy or not: the
// reference does not mix the clear column into the emission contribution function.
// ---------------------------------------------------------------------------
template <bool kCloudy>
struct EmissionColumn {
    const double *ec;       // this column of the walker's ec: stride nwave
    int64_t nwave;
    double w, factor;
    double acc, prev, eprev;
    bool stopped;
    CloudWalk cloud;        // (kCloudy)

    __device__ __forceinline__ double at(int k) const
    {
        if constexpr (kCloudy)
            return ec[(int64_t)k * nwave] + cloud.at(k);
        else
            return ec[(int64_t)k * nwave];
    }
    __device__ __forceinline__ void start(int itop)
    {
        acc = 0.0;
        eprev = 1.0;                                    // exp(-0): rows up to itop
        stopped = false;
        prev = at(itop);
    }
    // cf[k] before the normalisation, k = 0 .. L-2 in order
    __device__ __forceinline__ double step(int k, const double *s_kt, const double *s_h,
                                           const double *s_dlp, double maxdepth, int itop,
                                           int ibottom, int nlayers)
    {
        double enext = 1.0;                             // rows up to itop and below the stop: depth 0
        if (k + 1 > itop && !stopped) {
            const double cur = at(k + 1);
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

// the clouds of the kCloudy instantiation: deck_itop / deck_tsurf [nwalkers] or null (no deck)
struct EmissionClouds {
    const int32_t *deck_itop;
    const double *deck_tsurf;
    pb_cloud_terms cl;
};

template <bool kCloudy>
__global__ __launch_bounds__(kBlock) void k_band_cf_emission(
    double *__restrict__ parts, const double *__restrict__ ec, const double *__restrict__ intervals,
    const double *__restrict__ dlogp, const double *__restrict__ wn,
    const double *__restrict__ temps, const int32_t *__restrict__ band_start,
    const int32_t *__restrict__ band_count, const double *__restrict__ response,
    const int64_t *__restrict__ response_offset, double maxdepth, int itop, int ibottom,
    int nlayers, int nwave, EmissionClouds clouds)
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

    EmissionColumn<kCloudy> c;
    if constexpr (kCloudy) {
        if (clouds.deck_itop) {                         // (wave-uniform: the walker's deck)
            const int dk = pb::deck_layer(clouds.deck_itop, wk, nlayers);
            ibottom = dk + 1;
            if (threadIdx.x == 0)
                pb::sane_divisor(pb::kKB * uniform_f64(clouds.deck_tsurf + wk), s_kt[dk],
                                 s_kt[nlayers + dk]);
            __syncthreads();
        }
        c.cloud.init(clouds.cl, wk, s.live ? s.g : 0, nlayers);
    }
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
// Transit geometry with clouds, FROM ec (pyrat_obj.py:135-139, 683-689; optic_depth.py:94-121 with
// the early exit of _trapezoid.c:259-273): per walker a clear column, ec over the rows itop .. L-1,
// and a cloudy one, ec + ec_cloud over the rows itop .. deck_itop (no deck: L-1).  In each,
//   ideep = the first row whose depth exceeds maxdepth, else the column's last row
//           (deck_itop <= itop: itop -- no cloudy row at all)
//   T[r]  = 1 above itop, exp(-depth[r]) for itop <= r < ideep, 0 from ideep on
// and the layer's value is f T_cloudy + (1 - f) T_clear (f_patchy NULL: T_cloudy, and the clear
// column is not walked), times response x trapezoid weight.  The deck's radius does not enter.
// The walk is pb_cloud_walk.h's: a thread owns a column, the impact parameters are taken
// kCloudyRows at a time with the block's ray-path segments staged in LDS (stage_path_block), the
// rows' optical depths formed by depth_block; kTwo: ec_cloud != 0, else one running sum serves
// both columns.  Row by row the wavefront's sum
// goes into the LDS row store_parts reads; the rows after every column of the workgroup has closed
// are written too (a closed row is f 0 + (1 - f) 0: 0, or NaN with f).  (Reducing the 16 rows of
// a block together -- 17 shuffles instead of 96 -- was measured SLOWER, 6.9 against 5.0 ms at
// C5's shape: profiles/contribution.md.)
// ---------------------------------------------------------------------------
struct CloudyBandArgs {
    double *parts;
    const double *ec, *wn, *raypath;
    int64_t path_stride;
    const int32_t *band_start, *band_count;
    const double *response;
    const int64_t *response_offset;
    const int32_t *deck_itop;                  // [nwalkers] or null: no deck
    const double *f_patchy;                    // [nwalkers] or null: the cloudy column alone
    double maxdepth;
    int itop, nlayers, nwave;
    pb_cloud_terms cl;
};

template <bool kTwo>
__global__ __launch_bounds__(kBlock) void k_band_transmittance_cloudy(CloudyBandArgs a)
{
    constexpr int kRows = kCloudyRows;
    extern __shared__ __align__(16) double s_lds[];     // [kWaves][L] sums, [segment][kRows] paths
    const Sample s = band_sample(a.band_start, a.band_count, a.nwave);
    if (blockIdx.x * kBlock >= s.retained)
        return;
    const int nlayers = a.nlayers, nwave = a.nwave, itop = a.itop;
    double *s_path = s_lds + kWaves * nlayers;
    const int wk = blockIdx.z;
    const double *path = a.raypath + (int64_t)wk * a.path_stride;
    const bool need_clear = a.f_patchy != nullptr;
    // wave-uniform: the walker's deck and cloudy fraction
    const int dk = a.deck_itop ? pb::deck_layer(a.deck_itop, wk, nlayers) : nlayers - 1;
    const int nrow = nlayers - itop;
    const int nimp_c = dk + 1 - itop;                   // rows of the cloudy column (<= 0: none)
    const int nimp_l = need_clear ? nrow : 0;
    const int nimp = max(max(nimp_c, nimp_l), 0);
    const double f = need_clear ? pb::patchy_fraction(a.f_patchy, wk) : 0.0;
    const auto mix = [&](double cloudy, double clear) {
        return need_clear ? pb::patchy_mix(f, cloudy, clear) : cloudy;
    };
    const double scale = s.live ? a.response[a.response_offset[blockIdx.y] + s.i] *
                                      band_weight(a.wn, s.g, s.i, s.count, nwave)
                                : 0.0;
    const double *src = a.ec + ((int64_t)wk * nlayers + itop) * nwave + (s.live ? s.g : 0);
    CloudWalk cloud;
    if constexpr (kTwo)
        cloud.init(a.cl, wk, s.live ? s.g : 0, nlayers);
    double *red = s_lds + (threadIdx.x / kWave) * nlayers;
    const int lane = threadIdx.x & (kWave - 1);

    // the rows above itop: depth 0 in both columns
    {
        const double v = wave_sum(s.live ? mix(1.0, 1.0) * scale : 0.0);
        if (lane == 0)
            for (int r = 0; r < itop; r++)
                red[r] = v;
    }
    bool open_l = s.live && nimp_l > 0, open_c = s.live && nimp_c > 0;
    int rb = 0;
    for (; rb < nimp; rb += kRows) {
        // every column of the workgroup has closed both of its integrals: nothing left to compute
        if (__syncthreads_count(open_l || open_c) == 0)
            break;
        const int rlast = min(rb + kRows, nimp) - 1;
        pb::stage_path_block<kRows, kBlock>(s_path, path, rb, rlast);
        __syncthreads();
        double tau[kRows] = {}, tau_c[kTwo ? kRows : 1] = {};   // (both columns closed: no walk)
        if (open_l || open_c)
            pb::depth_block<kRows, kTwo>(tau, tau_c, src, nwave, rlast, s_path, cloud, itop);
        // (every lane of the wavefront takes every row: the sums are wave-wide)
#pragma unroll
        for (int k = 0; k < kRows; k++) {
            const int r = rb + k;
            if (r > rlast)
                continue;
            const double t = tau[k];
            const double t_c = kTwo ? tau_c[k] : t;
            const bool do_l = open_l && r < nimp_l, do_c = open_c && r < nimp_c;
            double e = 0.0, t_clear = 0.0, t_cloudy = 0.0;
            if (do_l || (!kTwo && do_c))
                e = pb::exp_s(-t);
            if (do_l) {
                if (t > a.maxdepth || r == nimp_l - 1)
                    open_l = false;                         // this row is the column's ideep
                else
                    t_clear = e;
            }
            if (do_c) {
                if (t_c > a.maxdepth || r == nimp_c - 1)
                    open_c = false;
                else
                    t_cloudy = kTwo ? pb::exp_s(-t_c) : e;
            }
            const double v = wave_sum(s.live ? mix(t_cloudy, t_clear) * scale : 0.0);
            if (lane == 0)
                red[itop + r] = v;
        }
    }
    // the rows no column of the workgroup reached
    {
        const double v = wave_sum(s.live ? mix(0.0, 0.0) * scale : 0.0);
        if (lane == 0)
            for (int r = min(rb, nimp); r < nrow; r++)
                red[itop + r] = v;
    }
    store_parts(a.parts, s_lds, nlayers);
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

// What the four entry points refuse alike, in the order they refuse it: the sizes, the layer cap,
// itop, ibottom (an entry without one passes 0), 65535 bands / walkers; then what the entry checks
// on its own (`own`); then -- unless there is nothing to do: *nchunks = -1 -- the null pointers
// (`pointers`: the entry's list) and the work buffer.
template <class Own>
int check_band_call(const char *who, int min_layers, int max_layers, int itop, int ibottom,
                    int nlayers, int nwave, int nbands, int nwalkers, int max_band_count,
                    bool pointers, const double *work_d, int *nchunks, Own own)
{
    *nchunks = -1;
    PB_REQUIRE(nlayers >= min_layers && nwave >= 1 && nbands >= 0 && nwalkers >= 0 &&
                   max_band_count >= 0,
               "%s: bad sizes%s", who, min_layers == 2 ? " (nlayers >= 2, nwave >= 1)" : "");
    PB_REQUIRE(nlayers <= max_layers, "%s: %d layers, at most %d fit in the LDS of a workgroup",
               who, nlayers, max_layers);
    PB_REQUIRE(itop >= 0 && itop < nlayers, "%s: itop out of range", who);
    PB_REQUIRE(ibottom <= nlayers, "%s: ibottom > nlayers", who);
    PB_REQUIRE(nbands <= 65535 && nwalkers <= 65535,
               "%s: at most 65535 bands and walkers per call", who);
    if (int rc = own())
        return rc;
    if (nbands == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(pointers, "%s: null pointer", who);
    *nchunks = pb::div_up(max_band_count, kBlock);
    PB_REQUIRE(*nchunks == 0 || work_d, "%s: null work buffer", who);
    return PB_OK;
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

// The two emission entries: kCloudy takes the deck's pointers (both or neither) and the cloud
// terms (or null).  Two instantiations, since the clear one needs 45 VGPRs against 67.
template <bool kCloudy>
int band_cf_emission(const char *who, double *out_d, const double *ec_d, const double *intervals_d,
                     const double *dlogp_d, const double *wn_d, const double *temps_d,
                     const int32_t *band_start_d, const int32_t *band_count_d,
                     const double *response_d, const int64_t *response_offset_d,
                     int max_band_count, double maxdepth, int itop, int ibottom, int nlayers,
                     int nwave, int nbands, int nwalkers, const int32_t *deck_itop_d,
                     const double *deck_tsurf_d, const pb_cloud_terms *cloud, double *work_d,
                     void *stream)
{
    int nchunks;
    const int rc = check_band_call(
        who, 2, kMaxLayersEmission, itop, ibottom, nlayers, nwave, nbands, nwalkers,
        max_band_count,
        out_d && ec_d && intervals_d && dlogp_d && wn_d && temps_d && band_start_d &&
            band_count_d && response_d && response_offset_d,
        work_d, &nchunks, [&]() -> int {
            if (!kCloudy)
                return PB_OK;
            PB_REQUIRE(!deck_itop_d == !deck_tsurf_d,
                       "%s: deck_itop_d and deck_tsurf_d go together", who);
            return pb::check_cloud(cloud, who);
        });
    if (rc || nchunks < 0)
        return rc;
    if (nchunks > 0) {
        EmissionClouds clouds{deck_itop_d, deck_tsurf_d, {}};
        if (cloud && cloud->nr > 0)
            clouds.cl = *cloud;
        const size_t lds = ((size_t)(4 + kWaves) * nlayers - 2) * sizeof(double);
        k_band_cf_emission<kCloudy>
            <<<dim3(nchunks, nbands, nwalkers), kBlock, lds, pb::as_stream(stream)>>>(
                work_d, ec_d, intervals_d, dlogp_d, wn_d, temps_d, band_start_d, band_count_d,
                response_d, response_offset_d, maxdepth, itop, ibottom, nlayers, nwave, clouds);
        PB_LAUNCH_CHECK();
    }
    return finish(out_d, work_d, band_start_d, band_count_d, nbands, nchunks, nlayers, nwave,
                  nwalkers, stream);
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
    return band_cf_emission<false>("pb_band_contribution_emission_batch", out_d, ec_d, intervals_d,
                                   dlogp_d, wn_d, temps_d, band_start_d, band_count_d, response_d,
                                   response_offset_d, max_band_count, maxdepth, itop, ibottom,
                                   nlayers, nwave, nbands, nwalkers, nullptr, nullptr, nullptr,
                                   work_d, stream);
}

int pb_band_transmittance_batch(double *out_d, const double *depth_d, const int32_t *ideep_d,
                                const double *wn_d, const int32_t *band_start_d,
                                const int32_t *band_count_d, const double *response_d,
                                const int64_t *response_offset_d, int max_band_count, int itop,
                                int nlayers, int nwave, int nbands, int nwalkers, double *work_d,
                                void *stream)
{
    const char *who = "pb_band_transmittance_batch";
    int nchunks;
    const int rc = check_band_call(
        who, 1, kMaxLayersTransit, itop, 0, nlayers, nwave, nbands, nwalkers, max_band_count,
        out_d && depth_d && ideep_d && wn_d && band_start_d && band_count_d && response_d &&
            response_offset_d,
        work_d, &nchunks, []() -> int { return PB_OK; });
    if (rc || nchunks < 0)
        return rc;
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

int pb_band_contribution_emission_cloudy_batch(
    double *out_d, const double *ec_d, const double *intervals_d, const double *dlogp_d,
    const double *wn_d, const double *temps_d, const int32_t *band_start_d,
    const int32_t *band_count_d, const double *response_d, const int64_t *response_offset_d,
    int max_band_count, double maxdepth, int itop, int ibottom, int nlayers, int nwave, int nbands,
    int nwalkers, const int32_t *deck_itop_d, const double *deck_tsurf_d,
    const pb_cloud_terms *cloud, double *work_d, void *stream)
{
    return band_cf_emission<true>("pb_band_contribution_emission_cloudy_batch", out_d, ec_d,
                                  intervals_d, dlogp_d, wn_d, temps_d, band_start_d, band_count_d,
                                  response_d, response_offset_d, max_band_count, maxdepth, itop,
                                  ibottom, nlayers, nwave, nbands, nwalkers, deck_itop_d,
                                  deck_tsurf_d, cloud, work_d, stream);
}

int pb_band_transmittance_cloudy_batch(double *out_d, const double *ec_d, const double *raypath_d,
                                       int64_t path_stride, const double *wn_d,
                                       const int32_t *band_start_d, const int32_t *band_count_d,
                                       const double *response_d,
                                       const int64_t *response_offset_d, int max_band_count,
                                       int itop, double maxdepth, int nlayers, int nwave,
                                       int nbands, int nwalkers, const int32_t *deck_itop_d,
                                       const pb_cloud_terms *cloud, const double *f_patchy_d,
                                       double *work_d, void *stream)
{
    const char *who = "pb_band_transmittance_cloudy_batch";
    const int64_t nrow = (int64_t)nlayers - itop, npath = (nrow * (nrow - 1)) / 2;
    int nchunks;
    const int rc = check_band_call(
        who, 1, kMaxLayersCloudyTransit, itop, 0, nlayers, nwave, nbands, nwalkers,
        max_band_count,
        out_d && ec_d && (raypath_d || npath == 0) && wn_d && band_start_d && band_count_d &&
            response_d && response_offset_d,
        work_d, &nchunks, [&]() -> int {
            PB_REQUIRE(path_stride == 0 || path_stride >= npath,
                       "%s: path_stride must be 0 or at least a walker's length", who);
            return pb::check_cloud(cloud, who);
        });
    if (rc || nchunks < 0)
        return rc;
    if (nchunks > 0) {
        // (no ray path at one impact parameter: the kernel then reads none)
        CloudyBandArgs a{work_d, ec_d, wn_d, raypath_d ? raypath_d : ec_d, path_stride,
                         band_start_d, band_count_d, response_d, response_offset_d, deck_itop_d,
                         f_patchy_d, maxdepth, itop, nlayers, nwave, {}};
        const bool two = cloud && cloud->nr > 0;
        if (two)
            a.cl = *cloud;
        const dim3 grid(nchunks, nbands, nwalkers);
        const size_t lds = ((size_t)kWaves * nlayers + (size_t)kCloudyRows * nrow) * sizeof(double);
        if (two)
            k_band_transmittance_cloudy<true><<<grid, kBlock, lds, pb::as_stream(stream)>>>(a);
        else
            k_band_transmittance_cloudy<false><<<grid, kBlock, lds, pb::as_stream(stream)>>>(a);
        PB_LAUNCH_CHECK();
    }
    return finish(out_d, work_d, band_start_d, band_count_d, nbands, nchunks, nlayers, nwave,
                  nwalkers, stream);
}

}  // extern "C"
