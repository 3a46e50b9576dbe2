// What the batched interpolation (pb_interp.hip) shares with its continuum epilogue
// (pb_interp_cont.hip) and with the one-pass table transit (pb_table_transit.hip): the
// per-(walker, layer) brackets and weights of k_interp_weights and the workspace of a call.
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

// The workspace of a pb_interp_ec_batch* call, n = nwalkers * nlayers, in doubles:
//   coef[n][2 * ncoef] | tlo[n] (int32) | rec[n][nrec] | Lecavelier rows [nlec][nwalkers][nwave]
// coef and tlo are the weights above.  The continuum's per-(walker, layer) records start where the
// weights of eight species end (16 n + ceil(n / 2), and a double between), whatever ncoef is; its
// per-walker Lecavelier rows follow them (pb_interp_cont.hip writes both).  Without a continuum
// the call needs what lies before `rec`; the sizes keep the slack callers have always allocated.
struct InterpWork {
    double *coef;
    int32_t *tlo;
    double *rec, *rows;
};

inline int64_t interp_work_rec(int64_t n) { return n * 16 + (n + 1) / 2 + 1; }

inline InterpWork interp_work(void *work_d, int64_t n, int ncoef, int nrec)
{
    double *coef = reinterpret_cast<double *>(work_d);
    double *rec = coef + interp_work_rec(n);
    return InterpWork{coef, interp_tlo(coef, n, ncoef), rec, rec + n * nrec};
}

// doubles of a call without a continuum, and of one with records of nrec doubles and nlec rows
inline int64_t interp_work_doubles(int64_t n) { return 17 * n + 8; }
inline int64_t interp_work_doubles(int64_t n, int nrec, int64_t nlec, int nwalkers, int nwave)
{
    return interp_work_rec(n) + n * nrec + nlec * nwalkers * nwave + 8;
}

// k_interp_weights into that workspace
int launch_interp_weights(double *coef, const double *ttable_d, const double *temps_d,
                          const double *density_d, int nmol, int ntemp, int64_t n, hipStream_t s);

}  // namespace pbi
