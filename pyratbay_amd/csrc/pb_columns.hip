// Numeric helpers over columns (a thread owns a wavenumber sample of a row-major
// [row][wavenumber] array): the device forms of cutils.ediff, _trapezoid.trapezoid2D and
// _simpson.simps2D.  The radiative-transfer kernels that used to live here: pb_transit_one.hip,
// pb_emission.hip, pb_two_stream.hip.
//
// Reference functions restated (pyratbay v2.0.1): src_c/cutils.c:27-42,
// src_c/_trapezoid.c:70-90, src_c/_simpson.c:167-203.
#include "pb_common.h"

namespace {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------
// cutils.ediff
// ---------------------------------------------------------------------------
__global__ void k_ediff(double *out, const double *arr, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 < n)
        out[i] = arr[i + 1] - arr[i];
}

// ---------------------------------------------------------------------------
// _trapezoid.trapezoid2D (src_c/_trapezoid.c:70-90)
// ---------------------------------------------------------------------------
__global__ void k_trapezoid2d(double *out, const double *data, const double *h,
                              const int32_t *nint, int nrows, int nwave)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nwave)
        return;
    int n = nint[j];
    if (n > nrows - 1)
        n = nrows - 1;      // the reference would read past the array
    double acc = 0.0;
    if (n > 0) {
        double prev = data[j];
        for (int i = 0; i < n; i++) {
            double next = data[(int64_t)(i + 1) * nwave + j];
            acc += h[i] * (prev + next);
            prev = next;
        }
    }
    out[j] = acc * 0.5;
}

// ---------------------------------------------------------------------------
// _simpson.simps2D (src_c/_simpson.c:167-203, include/simpson.h:29-47)
// ---------------------------------------------------------------------------
__global__ void k_simps2d(double *out, const double *y, int ny, int nwave,
                          const double *h, const int32_t *nint, const double *hsum,
                          const double *hratio, const double *hfactor)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwave)
        return;
    int n = nint[i];
    if (n > ny)
        n = ny;
    double res;
    if (n < 2) {
        res = 0.0;
    } else if (n == 2) {
        res = h[0] * 0.5 * (y[i] + y[(int64_t)nwave + i]);
    } else {
        double acc = 0.0;
        for (int p = 0; p < (n - 1) / 2; p++) {
            int j = 2 * p;
            acc += (y[(int64_t)j * nwave + i] * (2.0 - 1.0 / hratio[p]) +
                    y[(int64_t)(j + 1) * nwave + i] * hfactor[p] +
                    y[(int64_t)(j + 2) * nwave + i] * (2.0 - hratio[p])) * hsum[p];
        }
        res = acc / 6.0;
        if (n % 2 == 0)
            res += h[n - 2] * 0.5 *
                   (y[(int64_t)(n - 2) * nwave + i] + y[(int64_t)(n - 1) * nwave + i]);
    }
    out[i] = res;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int pb_ediff(double *out_d, const double *arr_d, int n, void *stream)
{
    PB_REQUIRE(n >= 0, "pb_ediff: n < 0");
    if (n < 2)
        return PB_OK;
    PB_REQUIRE(out_d && arr_d, "pb_ediff: null pointer");
    k_ediff<<<pb::div_up(n - 1, kBlock), kBlock, 0, pb::as_stream(stream)>>>(out_d, arr_d, n);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_trapezoid2D(double *out_d, const double *data_d, const double *intervals_d,
                   const int32_t *nint_d, int nrows, int nwave, void *stream)
{
    PB_REQUIRE(nrows >= 1 && nwave >= 0, "pb_trapezoid2D: bad shape");
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(out_d && data_d && nint_d && (nrows == 1 || intervals_d),
               "pb_trapezoid2D: null pointer");
    k_trapezoid2d<<<pb::div_up(nwave, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        out_d, data_d, intervals_d, nint_d, nrows, nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_simps2D(double *out_d, const double *y_d, int ny, int nwave, const double *h_d,
               const int32_t *nint_d, const double *hsum_d, const double *hratio_d,
               const double *hfactor_d, void *stream)
{
    PB_REQUIRE(ny >= 0 && nwave >= 0, "pb_simps2D: bad shape");
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(out_d && nint_d && (ny == 0 || y_d), "pb_simps2D: null pointer");
    PB_REQUIRE(ny < 3 || (h_d && hsum_d && hratio_d && hfactor_d), "pb_simps2D: null h");
    k_simps2d<<<pb::div_up(nwave, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        out_d, y_d, ny, nwave, h_d, nint_d, hsum_d, hratio_d, hfactor_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
