// Walker-batched retrieval path (BASELINE config 5), first stage: the cross-section table
// interpolated for a batch of atmospheres, with the continuum and alkali terms added in its store.
//
// The reference evaluates one model per Pyrat.eval() call (pyratbay/pyrat/pyrat_obj.py:225-385):
// interp_ec over the cross-section table (opacity/line_sampling.py:394-463 ->
// src_c/_extcoeff.c:367-418), transit_path (atmosphere/atmosphere.py:782-802), the optical-depth
// loop (opacity/optic_depth.py:103-112 -> src_c/_trapezoid.c:238-276), transmission
// (spectrum/radiative_transfer.py:57-71) and band integration (spectrum/spec_tools.py:193-233).
// Here a batch of nw walkers goes through every stage in ONE launch each, the walker index being
// a grid dimension: no per-walker Python, no host synchronisation, and the cross-section table is
// read once per chunk of walkers instead of once per walker.
//
//   k_transit_path        raypath[w][r(r-1)/2 + i] from radius[w][L]            (pb_transit.hip)
//   k_interp_ec_batch     ec[w][L][W] = sum_s dens[w][L][s] * lerp_T(etable[s][.][L][W])
//   k_transit_fused       ec -> (depth, ideep, spectrum): tau for all impact parameters, the
//                         reference's early exit and the transmission integral in one pass
//                                                                               (pb_transit.hip)
//   k_band_integrate_batch bandflux[w][nbands]                                  (pb_bands.hip)
//
// This file also holds the partition functions of a batch of atmospheres (k_iso_partition) and the
// loader of sampled cross sections (k_resample_cs).
#include <algorithm>
#include <cstdlib>

#include "pb_common.h"
#include "pb_alkali_voigt.h"
#include "pb_interp.h"

namespace {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------
// Partition functions Z_i(T) of the isotopes of one TLI database at the layer temperatures of a
// batch of atmospheres (line_by_line.py:156-158: interp1d(db.temp, db.iso_pf[j], kind='slinear');
// :219-222: evaluated at the temperature profile on every extinction call).  SciPy's first-order
// spline is evaluated as its de Boor recurrence does (w = 1/(t_hi - t_lo); Z = z_lo (w (t_hi - T))
// + z_hi (w (T - t_lo)), interval t_lo <= T < t_hi, the last one closed): bit-equal to it.  A
// temperature outside the table is an error in the reference (interp1d raises): NaN is written
// and counted in *nbad.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_iso_partition(
    double *z, int64_t z_iso_stride, int64_t z_t_stride, const double *temp, int64_t ntemp,
    const double *ttab, int ntab, const double *pf, int niso, int32_t *nbad)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= ntemp)
        return;
    const double x = temp[t];
    if (!(x >= ttab[0] && x <= ttab[ntab - 1])) {
        for (int i = 0; i < niso; i++)
            z[i * z_iso_stride + t * z_t_stride] = __longlong_as_double(0x7ff8000000000000ll);
        if (nbad)
            atomicAdd(nbad, 1);
        return;
    }
    int lo = 0, hi = ntab - 1;                 // largest lo <= ntab - 2 with ttab[lo] <= x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ttab[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    const double xa = ttab[lo], xb = ttab[lo + 1];
    const double w = 1.0 / (xb - xa);
    const double h0 = w * (xb - x), h1 = w * (x - xa);
    for (int i = 0; i < niso; i++) {
        const double *row = pf + (int64_t)i * ntab;
        z[i * z_iso_stride + t * z_t_stride] = row[lo] * h0 + row[lo + 1] * h1;
    }
}

// ---------------------------------------------------------------------------
// Layers nobody reads (round 5).  With the columns of a retrieval batch in the depth order of a base
// model (TableSpectrum.order_columns) the row tile at which the transit kernel leaves a column is
// known in advance to within a layer or two: tile[b] = the last ROW TILE (16 impact parameters)
// the columns 256 b ... 256 b + 255 can need (base model's deepest crossing in the block + a
// margin).  The interpolation then writes the layers row0 ... row0 + 16 (tile[b] + 1) - 1 only
// (at C5's shape 80 % of ec: 0.8 GB of 4.1 GB per 64 walkers less), and the transit kernel, should
// a walker's column still be open beyond that tile, raises flags[walker] and flags[nwalkers]
// instead of reading what was never written.  `gate` (repair pass): a launch whose workgroups
// return at once unless the flag it points to is set -- the full interpolation gated on
// flags[nwalkers], the transit of walker w gated on flags[w] -- so the repair costs two nearly
// empty launches when nothing was flagged, and no host synchronisation ever.
// ---------------------------------------------------------------------------
using pb::TileLimit;
using pb::uniform_i32;
using pb::layer_wanted;

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

struct ContPlanArgs {
    double *rec;
    const double *temps, *density, *pars;
    int nlayers, ncs, pars_stride, nrec;
    int64_t n;
    pb_cont_batch c;
    int alk_off;
};

// per (walker, layer): the scalars the epilogue reads (layout: rank-1 factors | per CIA table
// bracket, dt, node gap, density product | H- beta[6], bf prefactor, ff postfactor, T, n_H n_e |
// per alkali line dsigma, lorentz^2, -C2/T, wing prefactor, core prefactor, species density)
__global__ __launch_bounds__(kBlock) void k_cont_plan(ContPlanArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n)
        return;
    const int l = (int)(i % a.nlayers);
    const int64_t w = i / a.nlayers;
    const double t = a.temps[i];
    const double *d = a.density + i * a.ncs;
    const double *p = a.pars + w * a.pars_stride;
    double *r = a.rec + i * a.nrec;
    for (int m = 0; m < a.c.nrank1; m++) {
        const int kind = a.c.rank1_kind[m];
        if (kind == 0) {
            r[m] = d[a.c.rank1_species[m]];
            continue;
        }
        const double pr = a.c.rank1_pressure_d[m][l];
        const double nominal = pr * kCbBar / t / kCbK;      // lecavelier.py / gray.py: p BAR/T/K
        if (kind == 1) {
            r[m] = nominal;
        } else {
            const int q = a.c.rank1_par[m];
            const double p_top = pow(10.0, p[q + 2]), p_bottom = pow(10.0, p[q + 1]);
            const double cs = pr >= p_bottom && pr <= p_top ? pow(10.0, p[q]) * a.c.rank1_s0[m]
                                                            : 0.0;
            r[m] = cs * nominal;
        }
    }
    double *rc = r + a.c.nrank1;
    for (int c = 0; c < a.c.ncia; c++) {
        // k_continuum's bracket rule (_spline.c:235-251) on the temperature clamped to the table
        const double *tt = a.c.cia_temps_d[c];
        const int n = a.c.cia_ntemp[c];
        const double temp = fmin(fmax(t, tt[0]), tt[n - 1]);
        int idx = pb::nearest_index(tt, temp, 0, n - 1);
        if (idx == n - 1 || temp < tt[idx])
            idx--;
        rc[4 * c] = (double)idx;
        rc[4 * c + 1] = tt[idx] != temp ? temp - tt[idx] : 0.0;
        rc[4 * c + 2] = tt[idx + 1] - tt[idx];
        double prod = d[a.c.cia_species[c][0]];          // np.prod over the species, in order
        for (int j = 1; j < a.c.cia_nspec[c]; j++)
            prod = prod * d[a.c.cia_species[c][j]];
        rc[4 * c + 3] = prod;
    }
    if (a.c.hminus) {
        double *rh = rc + 4 * a.c.ncia;
        const double tc = fmin(fmax(t, 1000.0), 10080.0);
        // (a loop the compiler keeps: the same pow() calls as k_continuum, no constant folding)
#pragma nounroll
        for (int k = 0; k < 6; k++)
            rh[k] = pow(sqrt(5040.0 / tc), (double)(k + 2));
        const double alpha = kCbH * kCbC / kCbK;
        rh[6] = 0.75 * pow(t, -1.5) * kCbK * exp(kCbWn0Bf * alpha / t);
        rh[7] = kCbK * tc;
        rh[8] = t;
        rh[9] = d[a.c.hm_species[0]] * d[a.c.hm_species[1]];
    }
    double *ra = r + a.alk_off;
    for (int m = 0; m < a.c.nalkali; m++) {
        const double kC2 = 1.4387768775039338, kC3 = 8.852821681767784e-13;    // _alkali.c
        const pb::AlkaliLayer al = pb::alkali_layer(t, a.c.alkali_pressure_d[l],
                                                    a.c.alkali_detuning[m], a.c.alkali_lpar[m]);
        const double dens = a.c.alkali_density_d[i * a.c.nalkali + m];
        const double wing = al.dsigma * sqrt(al.dsigma) * exp(kC2 * al.dsigma / t);
        for (int j = 0; j < a.c.alkali_nlines[m]; j++, ra += kCbAlkRec) {
            const double vd = pb::alkali_voigt_det(t, al, a.c.alkali_mass[m], a.c.alkali_wn0[m][j]);
            const double g = kC3 * a.c.alkali_gf[m][j] / a.c.alkali_part_func[m];
            ra[0] = al.dsigma;
            ra[1] = al.lorentz * al.lorentz;
            ra[2] = -kC2 / t;
            ra[3] = vd * g * wing;
            ra[4] = al.lorentz / pb::kPi * g;
            ra[5] = dens;
        }
    }
}

struct ContRowsArgs {
    double *rows;                    // [nlec][nwalkers][nwave]
    const double *wn, *pars;
    int nwave, nwalkers, pars_stride, nlec;
    int par[kCbRank1];
    double s0[kCbRank1], l0[kCbRank1];
};

// Lecavelier.calc_cross_section per walker: 10**p0 * s0 * (wn * l0)**(-p1)
__global__ __launch_bounds__(kBlock) void k_cont_rows(ContRowsArgs a)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int w = blockIdx.y, j = blockIdx.z;
    if (i >= a.nwave)
        return;
    const double *p = a.pars + (int64_t)w * a.pars_stride + a.par[j];
    a.rows[((int64_t)j * a.nwalkers + w) * a.nwave + i] =
        pow(10.0, p[0]) * a.s0[j] * pow(a.wn[i] * a.l0[j], -p[1]);
}

// ---------------------------------------------------------------------------
// interp_ec for a batch of walkers, assigning form.  Workgroup = (256 wavenumbers, layer,
// chunk of walkers).  Walkers of a chunk that share a temperature bracket share its two table
// slices: the brackets the chunk uses at this layer are walked in ascending order, the upper
// node of one bracket staying in registers as the lower node of the next; a walker is computed
// in the pass of its own bracket.  Per-(walker, layer) brackets and weights come from
// k_interp_weights (wave-uniform loads).  kS = species held in registers (<= 8).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_interp_weights(
    int32_t *tlo_out, double *coef_out, const double *ttable, const double *temps,
    const double *density, int nmol, int ncoef, int ntemp, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const double t = temps[i];
    // same bracket rule as k_interp_ec (src_c/_extcoeff.c:394-398), clamped at the table's ends
    int tlo = pb::nearest_index(ttable, t, 0, ntemp - 1);
    if (t < ttable[tlo] || tlo == ntemp - 1)
        tlo--;
    tlo = max(tlo, 0);
    const double span = ttable[tlo + 1] - ttable[tlo];
    const double a = (ttable[tlo + 1] - t) / span, c = (t - ttable[tlo]) / span;
    tlo_out[i] = tlo;
    // the products interp_ec forms per sample, once per (walker, layer): w_lo*d_j, w_hi*d_j
    double *co = coef_out + i * 2 * ncoef;
    for (int j = 0; j < ncoef; j++) {
        const double d = j < nmol ? density[i * nmol + j] : 0.0;
        co[j] = a * d;
        co[ncoef + j] = c * d;
    }
}

// kFull: nmol == kS, no per-species predicate (the coefficient loads of a walker then merge into
// one scalar load and one wait)
template <int kS, bool kFull, int kCont = 0, bool kAlk = false>
__global__ __launch_bounds__(kBlock) void k_interp_ec_batch(
    double *ec, const double *etable, const int32_t *tlo, const double *coef, int nmol,
    int ntemp, int nlayers, int nwave, int nwalkers, int chunk, TileLimit lim, ContEpi cont = {})
{
    if (!layer_wanted(lim, blockIdx.y, blockIdx.x * kBlock, blockIdx.x * kBlock + kBlock, nwave))
        return;
    // per-(walker, layer) brackets and coefficients are wave-uniform: through the constant
    // address space they are SCALAR loads (one s_load_dwordx16 per walker at four species)
    typedef const double __attribute__((address_space(4))) *ccoef_t;
    typedef const int32_t __attribute__((address_space(4))) *ctlo_t;
    const ctlo_t ctlo = (ctlo_t)(unsigned long long)tlo;
    const int k = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int w0 = blockIdx.z * chunk, w1 = min(w0 + chunk, nwalkers);
    // brackets used by the chunk at this layer
    int bmin = ntemp, bmax = -1;
    for (int w = w0; w < w1; w++) {
        const int b = ctlo[(int64_t)w * nlayers + k];
        bmin = min(bmin, b);
        bmax = max(bmax, b);
    }
    if (i >= nwave)
        return;
    const int64_t slice = (int64_t)nlayers * nwave;
    const double *tab = etable + (int64_t)k * nwave + i;      // + (j*ntemp + t)*slice
    double lo[kS], hi[kS];
#pragma unroll
    for (int j = 0; j < kS; j++)
        hi[j] = kFull || j < nmol ? tab[((int64_t)j * ntemp + bmin) * slice] : 0.0;
    ContState<kCont, kAlk> cst;
    if constexpr (kCont != 0)
        cont_init(cst, cont, i, nwave);
    for (int b = bmin; b <= bmax; b++) {
#pragma unroll
        for (int j = 0; j < kS; j++) {
            lo[j] = hi[j];
            hi[j] = kFull || j < nmol ? tab[((int64_t)j * ntemp + b + 1) * slice] : 0.0;
        }
        // (the walkers of bracket b as the set bits of a ballot over per-lane brackets -- no
        // scalar load and wait per walker and bracket -- measured slower: 1.21 against 1.11 ms)
        for (int w = w0; w < w1; w++) {
            const int64_t wk = (int64_t)w * nlayers + k;
            if (ctlo[wk] != b)
                continue;                                   // wave-uniform
            const ccoef_t co = (ccoef_t)(unsigned long long)(coef + wk * 2 * kS);
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < kS; j++)
                if (kFull || j < nmol)
                    acc += lo[j] * co[j] + hi[j] * co[kS + j];
            if constexpr (kCont != 0)
                acc = cont_apply(acc, cst, cont, i, w, wk, nwave);
            ec[wk * nwave + i] = acc;
        }
    }
}

// Two adjacent samples per thread (16 bytes per lane and access: 1 KiB per wavefront store instead of
// 512 B).  The rows of ec and of the table start at layer * nwave samples, 8-byte aligned only when
// nwave is odd, so the pairs start at the first EVEN absolute element of the row: the accesses are
// then 16-byte aligned; the odd sample in front of / behind the pairs is done by one lane on its own.
// NP = pair slots per thread, kBlock slots apart (every store instruction of a workgroup still
// covers 4 KiB of consecutive samples): NP = 2 halves the per-walker scalar loads, waits and
// branches per byte written (0.902 against 0.914 ms per 64 walkers at C5's shape, same bits).
template <int kS, bool kFull, int NP>
__global__ __launch_bounds__(kBlock) void k_interp_ec_batch2(
    double *ec, const double *etable, const int32_t *tlo, const double *coef, int nmol,
    int ntemp, int nlayers, int nwave, int nwalkers, int chunk, TileLimit lim)
{
    // (slots [x NP kBlock, (x + 1) NP kBlock) hold the samples 2 q - 1 ... 2 q + 1)
    if (!layer_wanted(lim, blockIdx.y, 2 * (int)blockIdx.x * NP * kBlock - 1,
                      2 * ((int)blockIdx.x + 1) * NP * kBlock + 1, nwave))
        return;
    typedef const double __attribute__((address_space(4))) *ccoef_t;
    typedef const int32_t __attribute__((address_space(4))) *ctlo_t;
    typedef double d2 __attribute__((ext_vector_type(2)));
    const ctlo_t ctlo = (ctlo_t)(unsigned long long)tlo;
    const int k = blockIdx.y;
    const int w0 = blockIdx.z * chunk, w1 = min(w0 + chunk, nwalkers);
    int bmin = ntemp, bmax = -1;
    for (int w = w0; w < w1; w++) {
        const int b = ctlo[(int64_t)w * nlayers + k];
        bmin = min(bmin, b);
        bmax = max(bmax, b);
    }
    const int64_t slice = (int64_t)nlayers * nwave;
    // first sample of the row whose absolute element index is even (all slices / walkers share
    // the parity when slice and nlayers * nwave are of one parity -- checked by the launcher)
    const int head = (int)(((int64_t)k * nwave) & 1);
    // slot q of a row: its first sample alone when the row starts at an odd element, then pairs
    int ii[NP];
    bool live[NP], pair[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int q = (blockIdx.x * NP + p) * kBlock + threadIdx.x;
        ii[p] = head ? (q == 0 ? 0 : 1 + 2 * (q - 1)) : 2 * q;
        live[p] = ii[p] < nwave;
        pair[p] = live[p] && !(head && q == 0) && ii[p] + 1 < nwave;
        if (!live[p])
            ii[p] = 0;                                      // (a valid address; never stored)
    }
    if (!live[0])
        return;                                             // (slots ascend with p)
    const double *tab = etable + (int64_t)k * nwave;
    d2 lo[NP][kS], hi[NP][kS];
    auto load = [&](int p, int j, int b) -> d2 {
        const double *ptr = tab + ii[p] + ((int64_t)j * ntemp + b) * slice;
        if (pair[p])
            return *reinterpret_cast<const d2 *>(ptr);
        d2 v;
        v.x = ptr[0];
        v.y = 0.0;
        return v;
    };
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int j = 0; j < kS; j++)
            hi[p][j] = kFull || j < nmol ? load(p, j, bmin) : d2{0.0, 0.0};
    for (int b = bmin; b <= bmax; b++) {
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int j = 0; j < kS; j++) {
                lo[p][j] = hi[p][j];
                hi[p][j] = kFull || j < nmol ? load(p, j, b + 1) : d2{0.0, 0.0};
            }
        for (int w = w0; w < w1; w++) {
            const int64_t wk = (int64_t)w * nlayers + k;
            if (ctlo[wk] != b)
                continue;                                   // wave-uniform
            const ccoef_t co = (ccoef_t)(unsigned long long)(coef + wk * 2 * kS);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                d2 acc = {0.0, 0.0};
#pragma unroll
                for (int j = 0; j < kS; j++)
                    if (kFull || j < nmol) {
                        // same products and sums per sample as the one-sample kernel
                        acc.x += lo[p][j].x * co[j] + hi[p][j].x * co[kS + j];
                        acc.y += lo[p][j].y * co[j] + hi[p][j].y * co[kS + j];
                    }
                double *dst = ec + wk * nwave + ii[p];
                if (pair[p])
                    *reinterpret_cast<d2 *>(dst) = acc;
                else if (live[p])
                    dst[0] = acc.x;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Loader of sampled cross sections: one species' table of one opacity file brought onto the
// run's (temperature, pressure, wavenumber) grid -- tools.interpolate_opacity
// (pyratbay/tools/tools.py:1026-1107) as called by Line_Sample.__init__
// (opacity/line_sampling.py:245-275): linear in log(cs) over log(p), then over T, constant
// beyond the table; a zero cross section enters as exp(-230).  The brackets and weights of the
// two axes are prepared on the host (a handful of values); `wsel` are the kept wavenumber
// samples (window + thinning); `accumulate` adds to what the table holds (a species spread over
// several files is the sum of its files).  kResample = false: the grids agree with the file's,
// values are copied (or added) untouched, like the reference does.
// ---------------------------------------------------------------------------
template <bool kResample>
__global__ __launch_bounds__(kBlock) void k_resample_cs(
    double *out, const double *in, const int32_t *wsel, const int32_t *tlo, const double *ta,
    const int32_t *plo, const double *pa, int nlay_in, int nwave_in, int ntemp_out, int nlay_out,
    int nwave_out, int accumulate)
{
    const int w = blockIdx.x * kBlock + threadIdx.x;
    const int p2 = blockIdx.y, t2 = blockIdx.z;
    if (w >= nwave_out)
        return;
    const int64_t wi = wsel[w];
    auto at = [&](int t, int p) { return in[((int64_t)t * nlay_in + p) * nwave_in + wi]; };
    double v;
    if (!kResample) {
        v = at(tlo[t2], plo[p2]);
    } else {
        auto lg = [&](int t, int p) {
            const double y = log(at(t, p));
            return isfinite(y) ? y : -230.0;
        };
        auto over_p = [&](int t) {
            const double a = pa[p2];
            const int p = plo[p2];
            if (a == 0.0)
                return lg(t, p);
            const double lo = lg(t, p), hi = lg(t, p + 1);
            return lo + a * (hi - lo);                   // np.interp / slinear: lo + slope*(x - xlo)
        };
        const double b = ta[t2];
        const int t = tlo[t2];
        double y = over_p(t);
        if (b != 0.0) {
            const double hi = over_p(t + 1);
            y = y + b * (hi - y);
        }
        v = exp(y);
    }
    const int64_t o = ((int64_t)t2 * nlay_out + p2) * nwave_out + w;
    out[o] = accumulate ? out[o] + v : v;
}

}  // namespace

namespace pbi {

int launch_interp_weights(double *coef, const double *ttable_d, const double *temps_d,
                          const double *density_d, int nmol, int ntemp, int64_t n, hipStream_t s)
{
    const int ncoef = interp_ncoef(nmol);
    k_interp_weights<<<pb::div_up(n, kBlock), kBlock, 0, s>>>(interp_tlo(coef, n, ncoef), coef,
                                                            ttable_d, temps_d, density_d, nmol,
                                                            ncoef, ntemp, n);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace pbi

extern "C" {

int pb_iso_partition(double *z_d, int64_t z_iso_stride, int64_t z_t_stride,
                     const double *temp_d, int64_t ntemp, const double *ttab_d, int ntab,
                     const double *pf_d, int niso, int32_t *nbad_d, void *stream)
{
    PB_REQUIRE(ntemp >= 0 && niso >= 0 && ntab >= 2, "pb_iso_partition: bad shape (a partition-"
               "function table needs at least two temperatures, got %d)", ntab);
    if (ntemp == 0 || niso == 0)
        return PB_OK;
    PB_REQUIRE(z_d && temp_d && ttab_d && pf_d, "pb_iso_partition: null pointer");
    k_iso_partition<<<(unsigned)pb::div_up(ntemp, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        z_d, z_iso_stride, z_t_stride, temp_d, ntemp, ttab_d, ntab, pf_d, niso, nbad_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

// the alkali models' lines in all, or -1 if the counts are invalid
static int cont_alkali_lines(const pb_cont_batch *c)
{
    if (c->nalkali < 0 || c->nalkali > kCbAlk)
        return -1;
    int nl = 0;
    for (int m = 0; m < c->nalkali; m++) {
        if (c->alkali_nlines[m] < 1 || c->alkali_nlines[m] > kCbAlkLines)
            return -1;
        nl += c->alkali_nlines[m];
    }
    return nl <= kCbAlkLines ? nl : -1;
}

// where the alkali lines' records start in a (walker, layer) record
static int cont_alkali_offset(const pb_cont_batch *c)
{
    return c->nrank1 + 4 * c->ncia + 10 * c->hminus;
}

// the continuum's per-(walker, layer) record length (ContEpi::nrec), or -1 if `c` is invalid
static int cont_nrec(const pb_cont_batch *c)
{
    if (!c || c->nrank1 < 0 || c->nrank1 > kCbRank1 || c->ncia < 0 || c->ncia > kCbCia ||
        c->hminus < 0 || c->hminus > 1)
        return -1;
    const int nl = cont_alkali_lines(c);
    if (nl < 0)
        return -1;
    return cont_alkali_offset(c) + kCbAlkRec * nl;
}

static int cont_nlec(const pb_cont_batch *c)
{
    int n = 0;
    for (int m = 0; m < c->nrank1; m++)
        n += c->rank1_kind[m] == 1;
    return n;
}

// workspace of the continuum calls, in doubles: coef[n][16] | tlo[n] (int32) | rec[n][nrec] |
// Lecavelier rows [nlec][nwalkers][nwave]
static int64_t cont_rec_offset(int64_t n) { return n * 16 + (n + 1) / 2 + 1; }

static int cont_check(const pb_cont_batch *c)
{
    PB_REQUIRE(c, "pb_interp_ec_batch_cont: null continuum struct");
    PB_REQUIRE(c->nrank1 >= 0 && c->nrank1 <= kCbRank1,
               "pb_interp_ec_batch_cont: 0-%d rank-1 models, not %d", kCbRank1, c->nrank1);
    PB_REQUIRE(c->ncia >= 0 && c->ncia <= kCbCia,
               "pb_interp_ec_batch_cont: at most %d CIA tables, not %d", kCbCia, c->ncia);
    PB_REQUIRE(c->hminus == 0 || c->hminus == 1,
               "pb_interp_ec_batch_cont: at most one H- model, not %d", c->hminus);
    PB_REQUIRE(c->ncs >= 0 && c->npars >= 0 && (c->pars_stride == 0 || c->pars_stride == c->npars),
               "pb_interp_ec_batch_cont: bad counts (ncs %d, npars %d, pars_stride %d)", c->ncs,
               c->npars, c->pars_stride);
    bool need_dens = c->ncia > 0 || c->hminus;
    bool need_pars = false;
    for (int m = 0; m < c->nrank1; m++) {
        const int kind = c->rank1_kind[m];
        PB_REQUIRE(kind >= 0 && kind <= 2, "pb_interp_ec_batch_cont: rank-1 model %d: kind %d",
                   m, kind);
        if (kind == 0) {
            PB_REQUIRE(c->rank1_cs_d[m], "pb_interp_ec_batch_cont: null cross section (model %d)", m);
            PB_REQUIRE(c->rank1_species[m] >= 0 && c->rank1_species[m] < c->ncs,
                       "pb_interp_ec_batch_cont: rank-1 model %d: species %d of %d", m,
                       c->rank1_species[m], c->ncs);
            need_dens = true;
        } else {
            PB_REQUIRE(c->rank1_pressure_d[m], "pb_interp_ec_batch_cont: null pressure (model %d)", m);
            PB_REQUIRE(c->rank1_par[m] >= 0 && c->rank1_par[m] + (kind == 1 ? 2 : 3) <= c->npars,
                       "pb_interp_ec_batch_cont: rank-1 model %d: parameters %d.. of %d", m,
                       c->rank1_par[m], c->npars);
            need_pars = true;
        }
    }
    for (int k = 0; k < c->ncia; k++) {
        PB_REQUIRE(c->cia_tab_d[k] && c->cia_temps_d[k],
                   "pb_interp_ec_batch_cont: null CIA table %d", k);
        PB_REQUIRE(c->cia_ntemp[k] >= 2, "pb_interp_ec_batch_cont: CIA table %d: %d temperatures",
                   k, c->cia_ntemp[k]);
        PB_REQUIRE(c->cia_nspec[k] >= 1 && c->cia_nspec[k] <= kCbCia,
                   "pb_interp_ec_batch_cont: CIA table %d: 1-%d species, not %d", k, kCbCia,
                   c->cia_nspec[k]);
        for (int j = 0; j < c->cia_nspec[k]; j++)
            PB_REQUIRE(c->cia_species[k][j] >= 0 && c->cia_species[k][j] < c->ncs,
                       "pb_interp_ec_batch_cont: CIA table %d: species %d of %d", k,
                       c->cia_species[k][j], c->ncs);
    }
    PB_REQUIRE(c->ncia == 0 || c->cia_mask_d, "pb_interp_ec_batch_cont: null CIA mask");
    if (c->hminus) {
        PB_REQUIRE(c->hm_sigma_bf_d && c->hm_ff_d, "pb_interp_ec_batch_cont: null H- arrays");
        for (int j = 0; j < 2; j++)
            PB_REQUIRE(c->hm_species[j] >= 0 && c->hm_species[j] < c->ncs,
                       "pb_interp_ec_batch_cont: H- species %d of %d", c->hm_species[j], c->ncs);
    }
    PB_REQUIRE(c->nalkali >= 0 && c->nalkali <= kCbAlk,
               "pb_interp_ec_batch_cont: at most %d alkali models, not %d", kCbAlk, c->nalkali);
    int nlines = 0;
    for (int m = 0; m < c->nalkali; m++) {
        PB_REQUIRE(c->alkali_nlines[m] >= 1 && c->alkali_nlines[m] <= kCbAlkLines,
                   "pb_interp_ec_batch_cont: alkali model %d: 1-%d lines, not %d", m, kCbAlkLines,
                   c->alkali_nlines[m]);
        nlines += c->alkali_nlines[m];
        PB_REQUIRE(c->alkali_cutoff[m] > 0.0,
                   "pb_interp_ec_batch_cont: alkali model %d: cutoff %g (must be positive)", m,
                   c->alkali_cutoff[m]);
        PB_REQUIRE(c->alkali_part_func[m] > 0.0 && c->alkali_mass[m] > 0.0,
                   "pb_interp_ec_batch_cont: alkali model %d: partition function %g, mass %g", m,
                   c->alkali_part_func[m], c->alkali_mass[m]);
    }
    PB_REQUIRE(nlines <= kCbAlkLines,
               "pb_interp_ec_batch_cont: at most %d alkali lines in all, not %d", kCbAlkLines,
               nlines);
    if (c->nalkali) {
        PB_REQUIRE(c->alkali_pressure_d, "pb_interp_ec_batch_cont: null alkali pressure");
        PB_REQUIRE(c->alkali_density_d, "pb_interp_ec_batch_cont: null alkali density");
    }
    PB_REQUIRE(!(c->hminus || cont_nlec(c) || c->nalkali) || c->wn_d,
               "pb_interp_ec_batch_cont: null wn");
    PB_REQUIRE(!need_dens || c->density_d, "pb_interp_ec_batch_cont: null continuum density");
    PB_REQUIRE(!need_pars || c->pars_d, "pb_interp_ec_batch_cont: null continuum parameters");
    return PB_OK;
}

static int interp_ec_batch_launch(double *ec_d, const double *etable_d, const double *ttable_d,
                                  const double *temps_d, const double *density_d, void *work_d,
                                  int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                                  TileLimit lim, void *stream, const pb_cont_batch *cont = nullptr);

int pb_interp_ec_batch(double *ec_d, const double *etable_d, const double *ttable_d,
                       const double *temps_d, const double *density_d, void *work_d, int nmol,
                       int ntemp, int nlayers, int nwave, int nwalkers, void *stream)
{
    return interp_ec_batch_launch(ec_d, etable_d, ttable_d, temps_d, density_d, work_d, nmol, ntemp,
                                  nlayers, nwave, nwalkers, TileLimit{nullptr, 0, nullptr}, stream);
}

int pb_interp_ec_batch_limited(double *ec_d, const double *etable_d, const double *ttable_d,
                               const double *temps_d, const double *density_d, void *work_d,
                               int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                               const int32_t *tile_limit_d, int row0, const int32_t *gate_d,
                               void *stream)
{
    PB_REQUIRE(row0 >= 0 && row0 < std::max(nlayers, 1), "pb_interp_ec_batch_limited: row0 out of range");
    return interp_ec_batch_launch(ec_d, etable_d, ttable_d, temps_d, density_d, work_d, nmol, ntemp,
                                  nlayers, nwave, nwalkers, TileLimit{tile_limit_d, row0, gate_d},
                                  stream);
}

int64_t pb_interp_ec_batch_cont_work_doubles(const pb_cont_batch *cont, int nlayers, int nwave,
                                             int nwalkers)
{
    const int nrec = cont_nrec(cont);
    if (nrec < 0 || nlayers < 0 || nwave < 0 || nwalkers < 0)
        return -1;
    const int64_t n = (int64_t)nwalkers * nlayers;
    return cont_rec_offset(n) + n * nrec + (int64_t)cont_nlec(cont) * nwalkers * nwave + 8;
}

int pb_interp_ec_batch_cont(double *ec_d, const double *etable_d, const double *ttable_d,
                            const double *temps_d, const double *density_d, void *work_d,
                            int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                            const pb_cont_batch *cont, void *stream)
{
    const int rc = cont_check(cont);
    if (rc != PB_OK)
        return rc;
    return interp_ec_batch_launch(ec_d, etable_d, ttable_d, temps_d, density_d, work_d, nmol, ntemp,
                                  nlayers, nwave, nwalkers, TileLimit{nullptr, 0, nullptr}, stream,
                                  cont);
}

int pb_interp_ec_batch_cont_limited(double *ec_d, const double *etable_d, const double *ttable_d,
                                    const double *temps_d, const double *density_d, void *work_d,
                                    int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                                    const pb_cont_batch *cont, const int32_t *tile_limit_d,
                                    int row0, const int32_t *gate_d, void *stream)
{
    const int rc = cont_check(cont);
    if (rc != PB_OK)
        return rc;
    PB_REQUIRE(row0 >= 0 && row0 < std::max(nlayers, 1),
               "pb_interp_ec_batch_cont_limited: row0 out of range");
    return interp_ec_batch_launch(ec_d, etable_d, ttable_d, temps_d, density_d, work_d, nmol, ntemp,
                                  nlayers, nwave, nwalkers, TileLimit{tile_limit_d, row0, gate_d},
                                  stream, cont);
}

static int interp_ec_batch_launch(double *ec_d, const double *etable_d, const double *ttable_d,
                                  const double *temps_d, const double *density_d, void *work_d,
                                  int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                                  TileLimit lim, void *stream, const pb_cont_batch *cont)
{
    PB_REQUIRE(nmol >= 1 && nmol <= 8 && ntemp >= 2 && nlayers >= 1 && nwave >= 0 &&
                   nwalkers >= 0,
               "pb_interp_ec_batch: bad shape (1-8 species, >= 2 table temperatures)");
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(ec_d && etable_d && ttable_d && temps_d && density_d && work_d,
               "pb_interp_ec_batch: null pointer");
    hipStream_t s = pb::as_stream(stream);
    const int64_t n = (int64_t)nwalkers * nlayers;
    // workspace: coef[n][2*ncoef] doubles, then tlo[n] ints
    double *coef = reinterpret_cast<double *>(work_d);
    int32_t *tlo = pbi::interp_tlo(coef, n, pbi::interp_ncoef(nmol));
    // (a gated repair pass runs on the workspace its first pass filled: same walkers, same weights)
    if (!lim.gate) {
        const int rc = pbi::launch_interp_weights(coef, ttable_d, temps_d, density_d, nmol, ntemp,
                                                  n, s);
        if (rc != PB_OK)
            return rc;
    }
    // continuum: per-(walker, layer) scalars and per-walker Lecavelier rows behind the weights
    // (in the same workspace: a gated repair reuses them too)
    ContEpi epi{};
    int kcont = 0;
    bool kalk = false;
    if (cont) {
        const int nrec = cont_nrec(cont);
        double *rec = reinterpret_cast<double *>(work_d) + cont_rec_offset(n);
        double *rows = rec + n * nrec;
        const int nlec = cont_nlec(cont);
        if (!lim.gate) {
            if (nrec > 0) {
                ContPlanArgs pa{};
                pa.rec = rec;
                pa.temps = temps_d;
                pa.density = cont->density_d;
                pa.pars = cont->pars_d;
                pa.nlayers = nlayers;
                pa.ncs = cont->ncs;
                pa.pars_stride = cont->pars_stride;
                pa.nrec = nrec;
                pa.n = n;
                pa.c = *cont;
                pa.alk_off = cont_alkali_offset(cont);
                k_cont_plan<<<pb::div_up(n, kBlock), kBlock, 0, s>>>(pa);
                PB_LAUNCH_CHECK();
            }
            if (nlec > 0) {
                ContRowsArgs ra{};
                ra.rows = rows;
                ra.wn = cont->wn_d;
                ra.pars = cont->pars_d;
                ra.nwave = nwave;
                ra.nwalkers = nwalkers;
                ra.pars_stride = cont->pars_stride;
                ra.nlec = nlec;
                for (int m = 0, j = 0; m < cont->nrank1; m++)
                    if (cont->rank1_kind[m] == 1) {
                        ra.par[j] = cont->rank1_par[m];
                        ra.s0[j] = cont->rank1_s0[m];
                        ra.l0[j] = cont->rank1_l0[m];
                        j++;
                    }
                k_cont_rows<<<dim3(pb::div_up(nwave, kBlock), nwalkers, nlec), kBlock, 0, s>>>(ra);
                PB_LAUNCH_CHECK();
            }
        }
        epi.nrank1 = cont->nrank1;
        epi.ncia = cont->ncia;
        epi.nrec = nrec;
        for (int m = 0, j = 0; m < cont->nrank1; m++) {
            epi.kind[m] = cont->rank1_kind[m];
            if (epi.kind[m] == 0)
                epi.row[m] = cont->rank1_cs_d[m];
            else if (epi.kind[m] == 1)
                epi.row[m] = rows + (int64_t)(j++) * nwalkers * nwave;
        }
        for (int c = 0; c < cont->ncia; c++)
            epi.cia_tab[c] = cont->cia_tab_d[c];
        epi.cia_mask = cont->cia_mask_d;
        epi.wn = cont->wn_d;
        epi.hm_sigma_bf = cont->hm_sigma_bf_d;
        epi.hm_ff = cont->hm_ff_d;
        epi.rec = rec;
        epi.alk_off = cont_alkali_offset(cont);
        for (int m = 0; m < cont->nalkali; m++)
            for (int j = 0; j < cont->alkali_nlines[m]; j++, epi.alk_nl++) {
                epi.alk_wn0[epi.alk_nl] = cont->alkali_wn0[m][j];
                epi.alk_cutoff[epi.alk_nl] = cont->alkali_cutoff[m];
                if (j == cont->alkali_nlines[m] - 1)
                    epi.alk_end |= 1u << epi.alk_nl;
            }
        kcont = cont->hminus ? 2 : 1;
        kalk = cont->nalkali > 0;
    }
    // walkers per chunk: every chunk reads the table slices its walkers bracket again, so as many
    // as the launch can afford while it still fills the chip (C5, 64 walkers: 1.40 ms in chunks
    // of 16, 1.23 in one chunk, 1.11 with the species count a template constant)
    int chunk = 64;
    if (const char *e = getenv("PB_INTERP_CHUNK"))
        chunk = std::max(1, atoi(e));
    while (chunk > 1 && (int64_t)pb::div_up(nwave, kBlock) * nlayers * pb::div_up(nwalkers, chunk) < 2048)
        chunk /= 2;
    dim3 grid(pb::div_up(nwave, kBlock), nlayers, pb::div_up(nwalkers, chunk));
    // two samples per thread when every row of every slice / walker has the parity of its layer
    // index times nwave (slice = nlayers * nwave even, or nwave even), and 16-byte aligned bases
    static const bool pairs_on = !(getenv("PB_INTERP_PAIRS") && atoi(getenv("PB_INTERP_PAIRS")) == 0);
    const bool pairs = pairs_on && nwave >= 4 && (((int64_t)nlayers * nwave) % 2 == 0) &&
                       ((uintptr_t)ec_d % 16 == 0) && ((uintptr_t)etable_d % 16 == 0);
    // two pair slots per thread for launches that still fill the chip with half the workgroups
    // (up to four species: with eight, 146 registers would cost a wavefront per SIMD)
    int np = 1;
    if (pairs && nmol <= 4 && (int64_t)pb::div_up(nwave / 2 + 2, 2 * kBlock) * nlayers *
                         pb::div_up(nwalkers, chunk) >= 4096)
        np = 2;
    if (const char *e = getenv("PB_INTERP_NP"))
        np = atoi(e) == 2 ? 2 : 1;
    // with a continuum: one sample per thread.  The pair kernel with the epilogue needs 181 / 234
    // VGPRs (continuum / + H-: two wavefronts per SIMD) and ran slower at C5's shape: 1.48 against
    // 1.10 ms mean per launch, 4.35 against 3.69 ms per 64-walker transit step
    if (pairs && !kcont)
        grid.x = pb::div_up(nwave / 2 + 2, kBlock * np);
#define PB_INTERP_CONT(S, FULL, K)                                                             \
    do {                                                                                       \
        if (kalk)                                                                              \
            k_interp_ec_batch<S, FULL, K, true><<<grid, kBlock, 0, s>>>(                       \
                ec_d, etable_d, tlo, coef, nmol, ntemp, nlayers, nwave, nwalkers, chunk, lim, epi); \
        else                                                                                   \
            k_interp_ec_batch<S, FULL, K><<<grid, kBlock, 0, s>>>(                             \
                ec_d, etable_d, tlo, coef, nmol, ntemp, nlayers, nwave, nwalkers, chunk, lim, epi); \
    } while (0)
#define PB_INTERP(S, FULL)                                                                     \
    do {                                                                                       \
        if (kcont == 1)                                                                        \
            PB_INTERP_CONT(S, FULL, 1);                                                        \
        else if (kcont == 2)                                                                   \
            PB_INTERP_CONT(S, FULL, 2);                                                        \
        else if (pairs && np == 2)                                                                  \
            k_interp_ec_batch2<S, FULL, 2><<<grid, kBlock, 0, s>>>(ec_d, etable_d, tlo, coef,  \
                                                                   nmol, ntemp, nlayers, nwave, \
                                                                   nwalkers, chunk, lim);      \
        else if (pairs)                                                                        \
            k_interp_ec_batch2<S, FULL, 1><<<grid, kBlock, 0, s>>>(ec_d, etable_d, tlo, coef,  \
                                                                   nmol, ntemp, nlayers, nwave, \
                                                                   nwalkers, chunk, lim);      \
        else                                                                                   \
            k_interp_ec_batch<S, FULL><<<grid, kBlock, 0, s>>>(ec_d, etable_d, tlo, coef, nmol,  \
                                                               ntemp, nlayers, nwave, nwalkers, chunk, lim); \
    } while (0)
    static const bool no_full = getenv("PB_INTERP_FULL") && atoi(getenv("PB_INTERP_FULL")) == 0;
    if (nmol == 4 && !no_full)
        PB_INTERP(4, true);
    else if (nmol <= 4)
        PB_INTERP(4, false);
    else if (nmol == 8)
        PB_INTERP(8, true);
    else
        PB_INTERP(8, false);
#undef PB_INTERP
#undef PB_INTERP_CONT
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_resample_cross_section(double *out_d, const double *in_d, const int32_t *wsel_d,
                              const int32_t *tlo_d, const double *tweight_d,
                              const int32_t *plo_d, const double *pweight_d, int ntemp_in,
                              int nlay_in, int nwave_in, int ntemp_out, int nlay_out,
                              int nwave_out, int resample, int accumulate, void *stream)
{
    PB_REQUIRE(ntemp_in >= 1 && nlay_in >= 1 && nwave_in >= 1 && ntemp_out >= 1 && nlay_out >= 1 &&
                   nwave_out >= 0,
               "pb_resample_cross_section: bad shape");
    if (nwave_out == 0)
        return PB_OK;
    PB_REQUIRE(out_d && in_d && wsel_d && tlo_d && tweight_d && plo_d && pweight_d,
               "pb_resample_cross_section: null pointer");
    PB_REQUIRE(nlay_out <= 65535 && ntemp_out <= 65535, "pb_resample_cross_section: grid too large");
    dim3 grid(pb::div_up(nwave_out, kBlock), nlay_out, ntemp_out);
    if (resample)
        k_resample_cs<true><<<grid, kBlock, 0, pb::as_stream(stream)>>>(
            out_d, in_d, wsel_d, tlo_d, tweight_d, plo_d, pweight_d, nlay_in, nwave_in, ntemp_out,
            nlay_out, nwave_out, accumulate);
    else
        k_resample_cs<false><<<grid, kBlock, 0, pb::as_stream(stream)>>>(
            out_d, in_d, wsel_d, tlo_d, tweight_d, plo_d, pweight_d, nlay_in, nwave_in, ntemp_out,
            nlay_out, nwave_out, accumulate);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
