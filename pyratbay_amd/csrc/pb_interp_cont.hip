// The continuum and alkali epilogue of the batched interpolation, host side: the check of a
// caller's pb_cont_batch, the layout of the per-(walker, layer) records, and the two planning
// kernels that write what the epilogue (pb_interp_cont.h) reads -- k_cont_plan the records,
// k_cont_rows the per-walker Lecavelier rows.
#include "pb_common.h"
#include "pb_alkali_voigt.h"
#include "pb_interp_cont.h"

namespace {

using namespace pbi;

constexpr int kBlock = 256;

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

// where the alkali lines' records start in a (walker, layer) record
int cont_alkali_offset(const pb_cont_batch *c)
{
    return c->nrank1 + 4 * c->ncia + 10 * c->hminus;
}

// the counts that size a record, each against its bound; *nlines: the alkali models' lines in all
int cont_check_counts(const pb_cont_batch *c, int *nlines)
{
    PB_REQUIRE(c, "pb_interp_ec_batch_cont: null continuum struct");
    PB_REQUIRE(c->nrank1 >= 0 && c->nrank1 <= kCbRank1,
               "pb_interp_ec_batch_cont: 0-%d rank-1 models, not %d", kCbRank1, c->nrank1);
    PB_REQUIRE(c->ncia >= 0 && c->ncia <= kCbCia,
               "pb_interp_ec_batch_cont: at most %d CIA tables, not %d", kCbCia, c->ncia);
    PB_REQUIRE(c->hminus == 0 || c->hminus == 1,
               "pb_interp_ec_batch_cont: at most one H- model, not %d", c->hminus);
    PB_REQUIRE(c->nalkali >= 0 && c->nalkali <= kCbAlk,
               "pb_interp_ec_batch_cont: at most %d alkali models, not %d", kCbAlk, c->nalkali);
    *nlines = 0;
    for (int m = 0; m < c->nalkali; m++) {
        PB_REQUIRE(c->alkali_nlines[m] >= 1 && c->alkali_nlines[m] <= kCbAlkLines,
                   "pb_interp_ec_batch_cont: alkali model %d: 1-%d lines, not %d", m, kCbAlkLines,
                   c->alkali_nlines[m]);
        *nlines += c->alkali_nlines[m];
    }
    PB_REQUIRE(*nlines <= kCbAlkLines,
               "pb_interp_ec_batch_cont: at most %d alkali lines in all, not %d", kCbAlkLines,
               *nlines);
    return PB_OK;
}

}  // namespace

namespace pbi {

int cont_nrec(const pb_cont_batch *c)
{
    int nlines;
    if (cont_check_counts(c, &nlines) != PB_OK)
        return -1;
    return cont_alkali_offset(c) + kCbAlkRec * nlines;
}

int cont_nlec(const pb_cont_batch *c)
{
    int n = 0;
    for (int m = 0; m < c->nrank1; m++)
        n += c->rank1_kind[m] == 1;
    return n;
}

int cont_check(const pb_cont_batch *c)
{
    int nlines;
    const int rc = cont_check_counts(c, &nlines);
    if (rc != PB_OK)
        return rc;
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
    for (int m = 0; m < c->nalkali; m++) {
        PB_REQUIRE(c->alkali_cutoff[m] > 0.0,
                   "pb_interp_ec_batch_cont: alkali model %d: cutoff %g (must be positive)", m,
                   c->alkali_cutoff[m]);
        PB_REQUIRE(c->alkali_part_func[m] > 0.0 && c->alkali_mass[m] > 0.0,
                   "pb_interp_ec_batch_cont: alkali model %d: partition function %g, mass %g", m,
                   c->alkali_part_func[m], c->alkali_mass[m]);
    }
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

int cont_prepare(ContLaunch *out, const pb_cont_batch *cont, const InterpWork &work,
                 const double *temps_d, int nlayers, int nwave, int nwalkers, bool gated,
                 hipStream_t s)
{
    const int64_t n = (int64_t)nwalkers * nlayers;
    const int nrec = cont_nrec(cont);
    const int nlec = cont_nlec(cont);
    if (!gated) {
        if (nrec > 0) {
            ContPlanArgs pa{};
            pa.rec = work.rec;
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
            ra.rows = work.rows;
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
    ContEpi &epi = out->epi;
    epi = ContEpi{};
    epi.nrank1 = cont->nrank1;
    epi.ncia = cont->ncia;
    epi.nrec = nrec;
    for (int m = 0, j = 0; m < cont->nrank1; m++) {
        epi.kind[m] = cont->rank1_kind[m];
        if (epi.kind[m] == 0)
            epi.row[m] = cont->rank1_cs_d[m];
        else if (epi.kind[m] == 1)
            epi.row[m] = work.rows + (int64_t)(j++) * nwalkers * nwave;
    }
    for (int c = 0; c < cont->ncia; c++)
        epi.cia_tab[c] = cont->cia_tab_d[c];
    epi.cia_mask = cont->cia_mask_d;
    epi.wn = cont->wn_d;
    epi.hm_sigma_bf = cont->hm_sigma_bf_d;
    epi.hm_ff = cont->hm_ff_d;
    epi.rec = work.rec;
    epi.alk_off = cont_alkali_offset(cont);
    for (int m = 0; m < cont->nalkali; m++)
        for (int j = 0; j < cont->alkali_nlines[m]; j++, epi.alk_nl++) {
            epi.alk_wn0[epi.alk_nl] = cont->alkali_wn0[m][j];
            epi.alk_cutoff[epi.alk_nl] = cont->alkali_cutoff[m];
            if (j == cont->alkali_nlines[m] - 1)
                epi.alk_end |= 1u << epi.alk_nl;
        }
    out->kcont = cont->hminus ? 2 : 1;
    out->kalk = cont->nalkali > 0;
    return PB_OK;
}

}  // namespace pbi
