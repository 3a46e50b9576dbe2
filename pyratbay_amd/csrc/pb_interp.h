// What the one-pass table transit (pb_table_transit.hip) shares with the batched interpolation
// (pb_interp.hip): the per-(walker, layer) brackets and weights of k_interp_weights and the
// workspace they are written to.
#pragma once

#include "pb_common.h"

namespace pbi {

// coefficients per side of a bracket: the species count padded to what the kernels hold in registers
inline int interp_ncoef(int nmol) { return nmol <= 4 ? 4 : 8; }

// workspace of n = nwalkers * nlayers weights: coef[n][2 * ncoef] doubles, then tlo[n] ints
inline int32_t *interp_tlo(double *coef, int64_t n, int ncoef)
{
    return reinterpret_cast<int32_t *>(coef + n * 2 * ncoef);
}

// k_interp_weights into that workspace
int launch_interp_weights(double *coef, const double *ttable_d, const double *temps_d,
                          const double *density_d, int nmol, int ntemp, int64_t n, hipStream_t s);

}  // namespace pbi
