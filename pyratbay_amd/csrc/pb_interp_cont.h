// The continuum and alkali epilogue of the batched interpolation: the device side, which
// pb_interp.hip compiles into the store of k_interp_ec_batch, and the declarations of the host side
// (pb_interp_cont.hip), which checks the caller's struct and writes what the epilogue reads.
#pragma once

#include "pb_common.h"
#include "pb_interp.h"

namespace pbi {

// ---------------------------------------------------------------------------
// Continuum terms in the store of the batched interpolation (TableSpectrum.eval_bands with a
// Continuum).  A separate ec += continuum pass would read and write ec again (4.1 GB per 64
// walkers at C5's shape); instead the terms are added to `acc` in registers before it is stored.
// k_cont_plan writes per (walker, layer) the scalars of every term -- the rank-1 factors, the CIA
// brackets and density products, the H- temperature factors -- which the epilogue reads as
// wave-uniform scalar loads; k_cont_rows writes the one term that depends on both the sample and
// the walker's parameters, the Lecavelier cross section, once per walker.  The arithmetic and the
// order of the additions are those of Continuum.add -> k_continuum (pb_continuum.hip): rank-1
// models in list order, CIA tables in order, H-; per walker the result equals
// pb_interp_ec_batch followed by pb_continuum bit for bit for Rayleigh, CIA and H- (the
// Lecavelier / gray 10^x and pow run on the device, not in NumPy: within an ulp or two).
// kCont = 0: no continuum (the kernels compile to what they were); 1: continuum; 2: with H-.
//
// Alkali resonance doublets (kAlk, after H-: models in order, lines in order -- Continuum.add's
// pb_alkali_cross_section calls).  What made them a host job, the Voigt value at the detuning
// distance, is formed by k_cont_plan per (walker, layer, line) (pb_alkali_voigt.h: Re w(z) by a
// continued fraction, valid for Re z >= 20, which the caller guarantees).  Per line the record
// holds dsigma, lorentz^2, -C2/T, the wing prefactor voigt_det C3 gf/Z dsigma^1.5 exp(C2 dsigma/T),
// the core prefactor lorentz/pi C3 gf/Z and the species density; a thread keeps |wn - wn0|,
// |wn - wn0|^-1.5 and the inside-cutoff bit of its sample across the walker loop.  Per (walker,
// layer, sample, line) that leaves one exp (wing) or one division (core), no pow; k_alkali's
// branches exactly (_alkali.c:74-100), its values to rounding (the factors are grouped
// differently: a few ulp).  kAlk = false: the kernels compile to what they were.
// ---------------------------------------------------------------------------
constexpr int kCbRank1 = PB_CONT_MAX_RANK1;
constexpr int kCbCia = PB_CONT_MAX_CIA;
constexpr int kCbAlk = PB_CONT_MAX_ALKALI;
constexpr int kCbAlkLines = PB_CONT_MAX_ALKALI_LINES;
constexpr int kCbAlkRec = 6;       // doubles per (walker, layer, line)
constexpr int kCbRank1Reg = 4;     // Rayleigh cross sections kept in registers (more: re-read)
constexpr double kCbBar = 1e6;
constexpr double kCbK = 1.380649e-16, kCbH = 6.62607015e-27, kCbC = 29979245800.0;
constexpr double kCbWn0Bf = 6090.5;

struct ContEpi {
    int nrank1, ncia, nrec;
    int kind[kCbRank1];
    const double *row[kCbRank1];     // kind 0: [nwave]; kind 1: the walker rows [nwalkers][nwave]
    const double *cia_tab[kCbCia];   // [ntemp][nwave]
    const uint8_t *cia_mask;         // [nwave]
    const double *wn, *hm_sigma_bf, *hm_ff;
    const double *rec;               // [nwalkers * nlayers][nrec], written by k_cont_plan
    // alkali (kAlk): every model's lines in one list
    int alk_nl, alk_off;             // lines in all; where their records start in a rec row
    unsigned alk_end;                // bit j: line j is the last of its model
    double alk_wn0[kCbAlkLines], alk_cutoff[kCbAlkLines];
};

template <bool kAlk>
struct AlkState {};
template <>
struct AlkState<true> {
    double adwn[kCbAlkLines];        // |wn - wn0|
    double pw[kCbAlkLines];          // |wn - wn0|^-1.5
    unsigned in;                     // bit j: inside line j's cutoff
};

// the operands of a thread's sample that do not depend on the walker, kept across the walker loop
template <int kCont, bool kAlk = false>
struct ContState {
    double cs[kCbRank1Reg];
    unsigned mask;
    int cidx[kCbCia];                // wave-uniform: the CIA bracket whose rows are held
    double y0[kCbCia], sl[kCbCia];
    double wn, sig, ff[6];           // (kCont == 2)
    AlkState<kAlk> alk;
};

template <int kCont, bool kAlk>
__device__ __forceinline__ void cont_init(ContState<kCont, kAlk> &st, const ContEpi &a, int col,
                                          int nwave)
{
    if constexpr (kAlk) {
        const double wn = a.wn[col];
        st.alk.in = 0u;
#pragma unroll
        for (int j = 0; j < kCbAlkLines; j++) {
            const double dwn = j < a.alk_nl ? wn - a.alk_wn0[j] : 0.0;
            const double ad = fabs(dwn);
            st.alk.adwn[j] = ad;
            st.alk.pw[j] = 1.0 / (ad * sqrt(ad));
            // (_alkali.c:83: a sample beyond the cutoff on either side is skipped)
            if (j < a.alk_nl && !(dwn < -a.alk_cutoff[j] || dwn > a.alk_cutoff[j]))
                st.alk.in |= 1u << j;
        }
    }
#pragma unroll
    for (int m = 0; m < kCbRank1Reg; m++)
        st.cs[m] = m < a.nrank1 && a.kind[m] == 0 ? a.row[m][col] : 0.0;
    st.mask = a.ncia ? a.cia_mask[col] : 0u;
    if constexpr (kCont == 2) {
        st.wn = a.wn[col];
        st.sig = a.hm_sigma_bf[col];
#pragma unroll
        for (int i = 0; i < 6; i++)
            st.ff[i] = a.hm_ff[(int64_t)i * nwave + col];
    }
#pragma unroll
    for (int c = 0; c < kCbCia; c++)
        st.cidx[c] = -1;
}

// acc (the interpolated value of walker w, sample col) + every term, in Continuum.add's order
template <int kCont, bool kAlk>
__device__ __forceinline__ double cont_apply(double acc, ContState<kCont, kAlk> &st,
                                             const ContEpi &a, int col, int w, int64_t wk,
                                             int nwave)
{
    typedef const double __attribute__((address_space(4))) *crec_t;
    const crec_t r = (crec_t)(unsigned long long)(a.rec + wk * a.nrec);
    // rank-1: cross section x factor (k_continuum: ec += csv[m] * f[m][l])
#pragma unroll
    for (int m = 0; m < kCbRank1; m++) {
        if (m >= a.nrank1)
            break;
        const double f = r[m];
        const int kind = a.kind[m];
        double cs;
        if (kind == 0)
            cs = m < kCbRank1Reg ? st.cs[m] : a.row[m][col];
        else if (kind == 1)
            cs = a.row[m][(int64_t)w * nwave + col];
        else
            cs = 1.0;                       // (CCSgray: a row of ones in Continuum.add)
        acc += cs * f;
    }
    // CIA: the rows of the walker's bracket, held while the next walker shares it
    const crec_t rc = r + a.nrank1;
#pragma unroll
    for (int c = 0; c < kCbCia; c++) {
        if (c >= a.ncia)
            break;
        const int idx = (int)rc[4 * c];
        const double dt = rc[4 * c + 1], gap = rc[4 * c + 2], fp = rc[4 * c + 3];
        if (idx != st.cidx[c]) {                        // wave-uniform
            st.cidx[c] = idx;
            const double *t0 = a.cia_tab[c] + (int64_t)idx * nwave + col;
            const double y0 = t0[0], y1 = t0[nwave];
            st.y0[c] = y0;
            st.sl[c] = (y1 - y0) / gap;                 // (k_continuum: (y1 - y0) / inv)
        }
        if (st.mask >> c & 1u) {
            // a temperature on a node takes that row unchanged (dt = 0 there)
            const double cs = dt != 0.0 ? st.y0[c] + dt * st.sl[c] : st.y0[c];
            acc += cs * fp;
        }
    }
    if constexpr (kCont == 2) {
        const crec_t rh = rc + 4 * a.ncia;
        const double bfpre = rh[6], ffpost = rh[7], temp = rh[8], hf = rh[9];
        const double alpha = kCbH * kCbC / kCbK;
        const double bf = bfpre * (1.0 - exp(-st.wn * alpha / temp)) * st.sig;
        double ff = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++)
            if (st.ff[i] != 0.0)
                ff += rh[i] * st.ff[i];
        ff *= ffpost;
        acc += (bf + ff) * hf;
    }
    if constexpr (kAlk) {
        // per line: dsigma, lorentz^2, -C2/T, wing prefactor, core prefactor, density
        const crec_t ra = r + a.alk_off;
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < kCbAlkLines; j++) {
            if (j >= a.alk_nl)
                break;
            const crec_t q = ra + kCbAlkRec * j;
            if (st.alk.in >> j & 1u) {
                const double d = st.alk.adwn[j];
                if (d >= q[0])
                    sum += q[3] * st.alk.pw[j] * exp(q[2] * d);
                else
                    sum += q[4] / (q[1] + d * d);
            }
            if (a.alk_end >> j & 1u) {
                // (k_alkali: ec += acc * density, only where a line contributed)
                if (sum != 0.0)
                    acc += sum * q[5];
                sum = 0.0;
            }
        }
    }
    return acc;
}

// ---------------------------------------------------------------------------
// host side (pb_interp_cont.hip)
// ---------------------------------------------------------------------------

// PB_OK, or PB_ERR_ARG with a message: every bound and every pointer of a caller's struct
int cont_check(const pb_cont_batch *c);

// the per-(walker, layer) record length (ContEpi::nrec), or -1 if the counts of `c` are invalid;
// its Lecavelier models, one row per walker each
int cont_nrec(const pb_cont_batch *c);
int cont_nlec(const pb_cont_batch *c);

// what a launch needs of a checked struct: the kernel argument and the instantiation it selects
struct ContLaunch {
    ContEpi epi{};
    int kcont = 0;                   // 0: none, 1: continuum, 2: with H-
    bool kalk = false;
};

// k_cont_plan and k_cont_rows into work.rec and work.rows (not for a gated repair pass, which reuses
// what its first pass wrote there), and the ContLaunch that reads them
int cont_prepare(ContLaunch *out, const pb_cont_batch *cont, const InterpWork &work,
                 const double *temps_d, int nlayers, int nwave, int nwalkers, bool gated,
                 hipStream_t s);

}  // namespace pbi
