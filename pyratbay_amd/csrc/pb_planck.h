// Planck function of the column kernels (src_c/_blackbody.c:35-130), shared by pb_emission.hip,
// pb_two_stream.hip and pb_clouds.hip: every kernel forms B this way (same bits).
#pragma once

#include "pb_common.h"

namespace pb {

__device__ inline double planck_factor(double wn)
{
    return 2 * kH * kLS * kLS * pow(wn, 3.0);
}
// kt = kKB * temp and its rounded reciprocal: the same for every sample of a layer, so the
// column kernels prepare them once per (workgroup, layer) in LDS (planck_terms) and the exponent's
// division is pb::quot's three instructions
__device__ inline double planck_q(double factor, double wn, double kt, double inv_kt)
{
    return factor / (exp_s(quot_fast(kH * kLS * wn, kt, inv_kt)) - 1.0);
}
__device__ inline double planck(double factor, double wn, double temp)
{
    double kt, inv_kt;
    sane_divisor(kKB * temp, kt, inv_kt);      // (T = 0 -> B = 0 like the reference)
    return planck_q(factor, wn, kt, inv_kt);
}
// s_kt[0 .. 2 nlayers): kKB * temp[k] and 1 / (kKB * temp[k]) of one temperature profile, then
// 1 / mu[m] for the nmu quadrature angles (the angles themselves stay scalar loads)
__device__ inline void planck_terms(double *s_kt, const double *temp, int nlayers,
                                    const double *mu = nullptr, int nmu = 0)
{
    // (sane_divisor: a layer at T = 0 or a ray at mu = 0 keeps pb::quot_fast finite; the results
    // are those of the true divisions)
    for (int k = threadIdx.x; k < nlayers; k += blockDim.x)
        sane_divisor(kKB * temp[k], s_kt[k], s_kt[nlayers + k]);
    for (int m = threadIdx.x; m < nmu; m += blockDim.x) {
        double ms;
        sane_divisor(mu[m], ms, s_kt[2 * nlayers + m]);
    }
    __syncthreads();
}

}  // namespace pb
