// Ideal-gas densities and the hydrostatic radius (pyratbay/atmosphere/atmosphere.py:350-485,
// 629-664): the statements shared by the walker atmospheres (k_walker_atmosphere) and the
// radiative-equilibrium update (k_radeq_update) -- both kernels form them this way (same bits).
//
// CONSTANTS: pyratbay.constants (CODATA 2018 through scipy.constants, the products NumPy forms),
// which the reference's Python code -- ideal_gas_density, hydro_m, hydro_g -- runs with; not the
// legacy set of the C extensions in pb_common.h.
#pragma once

#include "pb_common.h"

namespace pb {
namespace atm {

constexpr double kBoltz = 1.380649e-23 * 1e7;    // pc.k = sc.k * 1e7 (erg K-1)
constexpr double kGrav = 6.67430e-11 * 1e3;      // pc.G = sc.G * 1e3 (dyne cm2 g-2)
constexpr double kAvogadro = 6.02214076e23;      // sc.N_A
constexpr double kBar = 1e6;                     // pc.bar (barye)

// ideal_gas_density: vmr * expand_dims(pressure / temperature) * pc.bar / pc.k (pressure in bar)
__device__ inline double ideal_gas_density(double vmr, double pressure_bar, double temp)
{
    return ((vmr * (pressure_bar / temp)) * kBar) / kBoltz;
}

// the integrand of the hydrostatic equation over ln p: rmodel 0 = hydro_m, 1 = hydro_g
__device__ inline double hydro_integrand(int rmodel, double temp, double mu, double mplanet,
                                         double gplanet)
{
    return rmodel == 0 ? ((kBoltz * kAvogadro) * temp) / ((kGrav * mu) * mplanet)
                       : ((-kBoltz * kAvogadro) * temp) / (mu * gplanet);
}

// cumulative trapezoid of the integrand over ln p, np.cumsum's order (left to right): ONE thread
__device__ inline void hydro_cumulative(double *s_int, const double *lnp, const double *s_aux,
                                        int nlayers)
{
    double run = 0.0;
    s_int[0] = 0.0;
    for (int l = 1; l < nlayers; l++) {
        run += (lnp[l] - lnp[l - 1]) * (s_aux[l] + s_aux[l - 1]) / 2.0;
        s_int[l] = run;
    }
}

// interp1d(pressure, I, kind='slinear')(p0), SciPy's first-order spline, for
// pressure[0] <= p0 <= pressure[nlayers - 1] (the caller's check)
__device__ inline double hydro_reference(const double *pressure, const double *s_int, double p0,
                                         int nlayers)
{
    int lo = 0, hi = nlayers;                    // searchsorted(pressure, p0, 'right')
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pressure[mid] <= p0)
            lo = mid + 1;
        else
            hi = mid;
    }
    lo = min(max(lo - 1, 0), nlayers - 2);
    const double pa = pressure[lo], pb = pressure[lo + 1];
    const double wgt = 1.0 / (pb - pa);
    return s_int[lo] * (wgt * (pb - p0)) + s_int[lo + 1] * (wgt * (p0 - pa));
}

__device__ inline double hydro_radius(int rmodel, double integral, double i0, double r0)
{
    return rmodel == 0 ? 1.0 / ((integral - i0) + 1.0 / r0) : integral + (r0 - i0);
}

}  // namespace atm
}  // namespace pb
