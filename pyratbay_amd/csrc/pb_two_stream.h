// Two-stream fluxes (pyratbay/pyrat/spectrum.py:454-522; Heng et al. 2014 Eqs. B5-B6): the
// statements of one layer interval, shared by the single-spectrum kernels (k_two_stream_trans,
// k_two_stream), the walker batch (k_two_stream_batch) and the net-flux batch
// (k_two_stream_net_batch, pb_radeq.hip) -- every kernel forms them this way (same bits).
// tests/test_gpu_two_stream_exact.py holds all four to 50-digit values of these formulas.
#pragma once

#include "pb_common.h"

namespace pb {

// exp1 = scipy.special.exp1 for real arguments (xsf/expint.h:22-52, the E1XB routine of
// Zhang & Jin 1996): power series for x <= 1, backward continued fraction otherwise.
__device__ inline double exp1_real(double x)
{
    const double ga = 0.5772156649015328606065120900824024;
    if (x == 0.0)
        return INFINITY;
    if (x <= 1.0) {
        double e1 = 1.0, r = 1.0;
        for (int k = 1; k < 26; k++) {
            const double k1 = k + 1.0;
            r = -r * k * x / (k1 * k1);
            e1 += r;
            if (fabs(r) <= fabs(e1) * 1e-15)
                break;
        }
        return -ga - log(x) + x * e1;
    }
    const int m = 20 + (int)(80.0 / x);
    double t0 = 0.0;
    for (int k = m; k > 0; k--)
        t0 = k / (1.0 + k / (x + t0));
    return exp_s(-x) * (1.0 / (x + t0));
}

// the diffusivity transmission of a layer interval of optical depth dtau0
__device__ inline double two_stream_trans(double dtau0)
{
    return (1 - dtau0) * exp_s(-dtau0) + dtau0 * dtau0 * exp1_real(dtau0);
}

// 1 - exp(-dtau0) of the sweeps' bracket, from expm1.  A deviation from the reference's bits
// (DESIGN.md): there the bracket -2/3 (1 - exp(-dtau0)) + dtau0 (1 - trans / 3) cancels from
// O(dtau0) to O(dtau0^2) while 1 - exp(-dtau0) carries an absolute error of 2^-53, and
// bp = dB / dtau0 multiplies what is left: pi |dB| 2^-53 / dtau0 per interval, O(1) of the flux at
// dtau0 = 1e-15.  With expm1 both terms of the bracket are good to their own size.
__device__ inline double two_stream_gone(double dtau0)
{
    return -expm1(-dtau0);
}

// downward sweep, interval (i, i+1): flux_down[i] -> flux_down[i+1]; btop = B[i], bbot = B[i+1]
__device__ inline double two_stream_down(double down, double trans, double dtau0, double btop,
                                         double bbot)
{
    const double pi = 3.141592653589793;
    const double bp = (bbot - btop) / dtau0;
    return trans * down + pi * btop * (1 - trans) +
           pi * bp * (-2.0 / 3 * two_stream_gone(dtau0) + dtau0 * (1 - trans / 3));
}

// upward sweep, interval (i, i+1): flux_up[i+1] -> flux_up[i]
__device__ inline double two_stream_up(double up, double trans, double dtau0, double btop,
                                       double bbot)
{
    const double pi = 3.141592653589793;
    const double bp = (bbot - btop) / dtau0;
    return trans * up + pi * bbot * (1 - trans) +
           pi * bp * (2.0 / 3 * two_stream_gone(dtau0) - dtau0 * (1 - trans / 3));
}

}  // namespace pb
