// High-resolution exit of eval() for a batch of walkers (pyrat/pyrat_obj.py:331-356):
//   ps.inst_convolution  = convolve(spectrum, taps, mode='same')   (spec_tools.py:817-880)
//   ps.rv_shift          = wn * sqrt((1 - v/c) / (1 + v/c))         (spec_tools.py:883-907)
//   si.interp1d(wn_shifted, convolved)(data_wn)                     (linear, bracket by searchsorted)
// pb_inst_convolve_batch writes the convolved spectra; pb_hires_observe_batch does all three steps
// per (walker, tile of the grid) without the convolved spectra ever reaching HBM.
//
// One workgroup stages kOut + (T - 1) samples of one walker in LDS (its outputs + (T - 1) / 2 on each
// side, zeros beyond the grid's ends like mode='same'), each sample scaled as it is loaded.  A lane
// accumulates outputs i, i + 256, ...: the lanes of a wave read consecutive doubles of the tile for
// every tap (ds_read_b64, conflict-free), the tap itself is wave-uniform (scalar load).  The sum
// runs over the taps in ascending order in both entry points: same bits from either.
#include "pb_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kOut = 1024;             // convolved samples per workgroup
constexpr int kPer = kOut / kBlock;    // per lane
constexpr int kMaxTaps = kOut + 1;     // halo (T - 1) / 2 <= kOut / 2 on each side
constexpr double kKm = 1.0e5;          // the reference's pc.km
constexpr double kC = 29979245800.0;   // the reference's pc.c (scipy.constants, CODATA 2018)

using pb::uniform_f64;

// s_l[m] = sample first + m of the walker's row (m < count), scaled; 0 outside [0, W)
__device__ __forceinline__ void stage_samples(double *s_l, const double *row, const double *scale,
                                              double walker_scale, int64_t first, int count, int W)
{
    for (int m = threadIdx.x; m < count; m += kBlock) {
        const int64_t p = first + m;
        double v = 0.0;
        if (p >= 0 && p < W) {
            v = row[p] * walker_scale;
            if (scale)
                v *= scale[p];
        }
        s_l[m] = v;
    }
}

// acc[j] = sum_t taps[t] * s_l[i_j + 2 H - t] for the lane's outputs i_j = lane + 256 j
__device__ __forceinline__ void conv_dense(double (&acc)[kPer], const double *s_l,
                                           const double *taps, int T)
{
#pragma unroll
    for (int j = 0; j < kPer; j++)
        acc[j] = 0.0;
    const double *p = s_l + (T - 1) + threadIdx.x;
    // The operands of tap t + 1 are requested before the products of tap t are issued.  (Not
    // unrolled over t: the reads of two consecutive taps are adjacent and would be fused into
    // ds_read2_b64, which moves a quarter of the bytes per LDS cycle of two ds_read_b64.)
    double k = uniform_f64(taps), s[kPer];
#pragma unroll
    for (int j = 0; j < kPer; j++)
        s[j] = p[j * kBlock];
#pragma unroll 1
    for (int t = 1; t < T; t++) {
        const double kn = uniform_f64(taps + t);
        double sn[kPer];
#pragma unroll
        for (int j = 0; j < kPer; j++)
            sn[j] = p[j * kBlock - t];
#pragma unroll
        for (int j = 0; j < kPer; j++) {
            acc[j] = fma(k, s[j], acc[j]);
            s[j] = sn[j];
        }
        k = kn;
    }
#pragma unroll
    for (int j = 0; j < kPer; j++)
        acc[j] = fma(k, s[j], acc[j]);
}

__device__ __forceinline__ double conv_one(const double *s_l, const double *taps, int T, int i)
{
    double acc = 0.0;
    const double *p = s_l + (T - 1) + i;
#pragma unroll 1
    for (int t = 0; t < T; t++)
        acc = fma(uniform_f64(taps + t), p[-t], acc);
    return acc;
}

__global__ __launch_bounds__(kBlock) void k_inst_convolve(
    double *__restrict__ out, const double *__restrict__ spectra, const double *__restrict__ taps,
    const double *__restrict__ sample_scale, int T, int W)
{
    extern __shared__ double lds[];
    double *s_l = lds;                                   // [kOut + T - 1]
    const int64_t g0 = (int64_t)blockIdx.x * kOut;
    const int64_t row = (int64_t)blockIdx.y * W;
    const int H = (T - 1) / 2;
    stage_samples(s_l, spectra + row, sample_scale, 1.0, g0 - H, kOut + T - 1, W);
    __syncthreads();
    double acc[kPer];
    conv_dense(acc, s_l, taps, T);
#pragma unroll
    for (int j = 0; j < kPer; j++) {
        const int64_t i = g0 + threadIdx.x + j * kBlock;
        if (i < W)
            out[row + i] = acc[j];
    }
}

// number of a[0 .. n) that are <= v (a ascending)
__device__ __forceinline__ int count_le(const double *a, int n, double v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// interp1d's bracket of d on the tile's shifted nodes x_l[0 .. nx): searchsorted(x, d, 'left')
// clipped to [1, W - 1], minus 1 -- as an offset into the tile (0 ... nx - 2)
__device__ __forceinline__ int bracket(const double *x_l, int nx, double d)
{
    int lo = 0, hi = nx;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x_l[mid] < d)
            lo = mid + 1;
        else
            hi = mid;
    }
    return min(max(lo - 1, 0), nx - 2);
}

// One workgroup: walker blockIdx.y, brackets [g0, g1) of the grid, g0 = blockIdx.x (kOut - 1): the
// data points whose bracket starts there need the convolved samples g0 ... g1 (<= kOut of them).
__global__ __launch_bounds__(kBlock) void k_hires_observe(
    double *__restrict__ out, const double *__restrict__ spectra, const double *__restrict__ wn,
    const double *__restrict__ taps, const double *__restrict__ sample_scale,
    const double *__restrict__ data, const int32_t *__restrict__ slot,
    const double *__restrict__ rv, const double *__restrict__ walker_scale, double rv_max, int T,
    int W, int ndata)
{
    extern __shared__ double lds[];
    double *s_l = lds;                                   // [kOut + T - 1] scaled samples
    double *c_l = s_l + (kOut + T - 1);                  // [kOut] convolved samples
    double *x_l = c_l + kOut;                            // [kOut] shifted nodes
    int *need = (int *)(x_l + kOut);                     // [kOut]
    int *list = need + kOut;                             // [kOut]
    __shared__ int range[2], count;

    const int w = blockIdx.y;
    const int g0 = blockIdx.x * (kOut - 1);
    const int g1 = min(g0 + kOut - 1, W - 1);
    const int nx = g1 - g0 + 1;                          // 2 ... kOut nodes
    const double v = rv ? rv[w] : 0.0;
    bool reject = !(fabs(v) <= rv_max);
    double f = 1.0;
    if (!reject) {
        const double vel = v * kKm;
        f = sqrt((1.0 - vel / kC) / (1.0 + vel / kC));
        // a data point off the shifted grid: interp1d raises, the walker is rejected
        reject = !(data[0] >= wn[0] * f && data[ndata - 1] <= wn[W - 1] * f);
        if (reject)
            f = 1.0;
    }
    // this tile's data points [range[0], range[1]): the tiles partition the sorted data at the
    // shifted nodes g0 (a point ON node g0 goes to the tile below: searchsorted 'left')
    if (threadIdx.x == 0)
        range[0] = g0 == 0 ? 0 : count_le(data, ndata, wn[g0] * f);
    if (threadIdx.x == 64)
        range[1] = g1 == W - 1 ? ndata : count_le(data, ndata, wn[g1] * f);
    for (int i = threadIdx.x; i < kOut; i += kBlock)
        need[i] = 0;
    if (threadIdx.x == 0)
        count = 0;
    __syncthreads();
    const int j0 = range[0], j1 = range[1];
    if (j0 >= j1)
        return;
    double *orow = out + (int64_t)w * ndata;
    if (reject) {
        for (int j = j0 + threadIdx.x; j < j1; j += kBlock) {
            const int s = slot[j];
            if ((unsigned)s < (unsigned)ndata)
                orow[s] = __builtin_huge_val();
        }
        return;
    }
    for (int i = threadIdx.x; i < nx; i += kBlock)
        x_l[i] = wn[g0 + i] * f;
    const int H = (T - 1) / 2;
    stage_samples(s_l, spectra + (int64_t)w * W, sample_scale, walker_scale ? walker_scale[w] : 1.0,
                  (int64_t)g0 - H, kOut + T - 1, W);
    __syncthreads();
    // the convolved samples somebody brackets
    for (int j = j0 + threadIdx.x; j < j1; j += kBlock) {
        const int lo = bracket(x_l, nx, data[j]);
        if (atomicExch(&need[lo], 1) == 0)
            list[atomicAdd(&count, 1)] = lo;
        if (atomicExch(&need[lo + 1], 1) == 0)
            list[atomicAdd(&count, 1)] = lo + 1;
    }
    __syncthreads();
    const int nneed = count;
    if (nneed * 4 > kOut) {
        double acc[kPer];
        conv_dense(acc, s_l, taps, T);
#pragma unroll
        for (int j = 0; j < kPer; j++)
            c_l[threadIdx.x + j * kBlock] = acc[j];
    } else {
        for (int k = threadIdx.x; k < nneed; k += kBlock) {
            const int i = list[k];
            c_l[i] = conv_one(s_l, taps, T, i);
        }
    }
    __syncthreads();
    for (int j = j0 + threadIdx.x; j < j1; j += kBlock) {
        const double d = data[j];
        const int lo = bracket(x_l, nx, d);
        const double x_lo = x_l[lo], x_hi = x_l[lo + 1];
        const double c_lo = c_l[lo], c_hi = c_l[lo + 1];
        const double slope = (c_hi - c_lo) / (x_hi - x_lo);
        const int s = slot[j];
        if ((unsigned)s < (unsigned)ndata)
            orow[s] = slope * (d - x_lo) + c_lo;
    }
}

size_t observe_lds_bytes(int T)
{
    return (size_t)(kOut + T - 1 + 2 * kOut) * sizeof(double) + (size_t)2 * kOut * sizeof(int);
}

}  // namespace

extern "C" {

int pb_inst_convolve_batch(double *out_d, const double *spectra_d, const double *taps_d,
                           const double *sample_scale_d, int ntaps, int nwave, int nwalkers,
                           void *stream)
{
    PB_REQUIRE(nwave >= 0 && nwalkers >= 0, "pb_inst_convolve_batch: bad shape");
    PB_REQUIRE(ntaps >= 1 && ntaps % 2 == 1, "pb_inst_convolve_batch: %d taps (an odd number >= 1 "
                                             "is needed)", ntaps);
    PB_REQUIRE(ntaps <= kMaxTaps, "pb_inst_convolve_batch: %d taps, at most %d are supported "
                                  "(one tile of %d samples + half a tile on each side)", ntaps,
               kMaxTaps, kOut);
    PB_REQUIRE(nwalkers <= 65535, "pb_inst_convolve_batch: more than 65535 walkers in one call");
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(out_d && spectra_d && taps_d, "pb_inst_convolve_batch: null pointer");
    PB_REQUIRE(out_d != spectra_d, "pb_inst_convolve_batch: not in place");
    dim3 grid(pb::div_up(nwave, kOut), nwalkers);
    k_inst_convolve<<<grid, kBlock, (size_t)(kOut + ntaps - 1) * sizeof(double),
                      pb::as_stream(stream)>>>(out_d, spectra_d, taps_d, sample_scale_d, ntaps,
                                               nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_hires_observe_batch(double *out_d, const double *spectra_d, const double *wn_d,
                           const double *taps_d, const double *sample_scale_d,
                           const double *data_wn_sorted_d, const int32_t *data_slot_d,
                           const double *rv_kms_d, const double *walker_scale_d, double rv_max,
                           int ntaps, int nwave, int ndata, int nwalkers, void *stream)
{
    PB_REQUIRE(nwave >= 2 && ndata >= 0 && nwalkers >= 0, "pb_hires_observe_batch: bad shape");
    PB_REQUIRE(ntaps >= 1 && ntaps % 2 == 1, "pb_hires_observe_batch: %d taps (an odd number >= 1 "
                                             "is needed)", ntaps);
    PB_REQUIRE(ntaps <= kMaxTaps, "pb_hires_observe_batch: %d taps, at most %d are supported "
                                  "(one tile of %d samples + half a tile on each side)", ntaps,
               kMaxTaps, kOut);
    PB_REQUIRE(nwalkers <= 65535, "pb_hires_observe_batch: more than 65535 walkers in one call");
    PB_REQUIRE(rv_max >= 0.0 && rv_max * kKm < kC, "pb_hires_observe_batch: rv_max = %g km/s",
               rv_max);
    if (ndata == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(out_d && spectra_d && wn_d && taps_d && data_wn_sorted_d && data_slot_d,
               "pb_hires_observe_batch: null pointer");
    dim3 grid(pb::div_up(nwave - 1, kOut - 1), nwalkers);
    k_hires_observe<<<grid, kBlock, observe_lds_bytes(ntaps), pb::as_stream(stream)>>>(
        out_d, spectra_d, wn_d, taps_d, sample_scale_d, data_wn_sorted_d, data_slot_d, rv_kms_d,
        walker_scale_d, rv_max, ntaps, nwave, ndata);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
