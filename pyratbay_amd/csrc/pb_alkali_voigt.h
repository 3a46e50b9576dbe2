// Voigt value of an alkali resonance line at the detuning distance, on the device -- the arithmetic
// of continuum.VanderWaals.voigt_det (pyratbay: opacity/alkali/alkali.py:48-82 ->
// opacity/broadening.py:231-260), one value per (layer, line).  Shared by
// pb_alkali_voigt_det_batch (pb_continuum.hip) and the batched continuum's k_cont_plan
// (pb_interp_cont.hip).
#ifndef PB_ALKALI_VOIGT_H
#define PB_ALKALI_VOIGT_H
#include <hip/hip_runtime.h>

namespace pb {

struct AlkaliLayer {
    double lorentz;     // lpar (T/2000)^-0.7 p / 1.01e6 (p in barye)
    double dsigma;      // detuning (T/500)^0.6
};

__device__ __forceinline__ AlkaliLayer alkali_layer(double temp, double pressure_barye,
                                                    double detuning, double lpar)
{
    AlkaliLayer a;
    a.lorentz = lpar * pow(temp / 2000.0, -0.7) * pressure_barye / 1010000.0;
    a.dsigma = detuning * pow(temp / 500.0, 0.6);
    return a;
}

// Re w(z) of the Faddeeva function by its Laplace continued fraction
//   w(z) = (i/sqrt(pi)) / (z - (1/2)/(z - 1/(z - (3/2)/(z - ...)))),
// the partial numerators 1/2, 1, ..., kLevels/2 evaluated bottom-up in plain FP64 complex
// arithmetic.  REGIME: Re z >= 20 (any Im z >= 0).  There 6 levels agree with
// scipy.special.wofz to 8e-15 relative (2e5 random points, Im z in [1e-10, 1e3]), and the real
// part is a sum of positive terms: no cancellation however small Im z.  The shipped models have
// Re z = dsigma/sigma = 570 ... 1069 (it grows as T^0.1); the callers refuse a model below 20.
constexpr int kFaddeevaLevels = 6;
constexpr double kFaddeevaMinX = 20.0;

__device__ __forceinline__ double faddeeva_re_far(double x, double y)
{
    double re = x, im = y;                  // r = z
#pragma unroll
    for (int k = kFaddeevaLevels; k >= 1; k--) {
        // r = z - (k/2) / r
        const double h = 0.5 * k, n = re * re + im * im;
        const double qre = h * re / n, qim = -h * im / n;
        re = x - qre;
        im = y - qim;
    }
    // (i/sqrt(pi)) / r = (i conj(r)) / (sqrt(pi) |r|^2): real part im / (sqrt(pi) |r|^2)
    return im / (1.7724538509055159 * (re * re + im * im));
}

// voigt_det of one (layer, line): the Faddeeva branch when lorentz/hwhm_G < 0.1, else the
// four-term rational approximation (broadening.py:249-259), selected per element
__device__ __forceinline__ double alkali_voigt_det(double temp, AlkaliLayer a, double mass,
                                                   double wn0)
{
    const double kK = 1.380649e-16, kAmu = 1.6605390666e-24, kC = 29979245800.0;
    const double kPi = 3.141592653589793, kLn2 = 0.6931471805599453;
    const double sqrt_ln2 = sqrt(kLn2);
    const double hg = sqrt(2.0 * kK * temp / (mass * kAmu)) * wn0 / kC;
    // the distance from the line centre as the reference forms it: (wn0 + dsigma) - wn0
    const double dx = (wn0 + a.dsigma) - wn0;
    if (a.lorentz / hg < 0.1) {
        const double sigma = hg / sqrt_ln2;
        return faddeeva_re_far(dx / sigma, a.lorentz / sigma) / (sigma * sqrt(kPi));
    }
    const double A[4] = {-1.2150, -1.3509, -1.2150, -1.3509};
    const double B[4] = {1.2359, 0.3786, -1.2359, -0.3786};
    const double Cc[4] = {-0.3085, 0.5906, -0.3085, 0.5906};
    const double D[4] = {0.0210, -1.1858, -0.0210, 1.1858};
    const double X = dx * sqrt_ln2 / hg, Y = a.lorentz * sqrt_ln2 / hg;
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
        v += (Cc[i] * (Y - A[i]) + D[i] * (X - B[i])) /
             ((Y - A[i]) * (Y - A[i]) + (X - B[i]) * (X - B[i]));
    return v * sqrt(kPi * kLn2) / (kPi * hg);
}

}  // namespace pb
#endif
