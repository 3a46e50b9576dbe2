// pb_walker_atmosphere: the walkers' atmospheres from their parameter vectors, one launch
// (Atmosphere.calc_profiles, pyratbay/pyrat/atmosphere.py:399-526, for a batch).
// pb_walker_atmosphere_chem is the same kernel on per-walker base VMRs (those of pb_equilibrium_vmr,
// pb_chemistry.hip, whose cell statuses it folds into the reject mask); pb_walker_temperature runs
// the T(p) model alone, for the equilibrium to read.
//
// One wavefront per walker, lanes over layers (looping when nlayers > 64), the profile in LDS.
// Everything in binary64, in the reference's order of operations; the build's -ffp-contract=off
// keeps products and sums apart like NumPy does.
//
// CONSTANTS: pyratbay.constants (pb_atm_profile.h, which also holds the ideal-gas and hydrostatic
// statements the radiative-equilibrium update shares), not the legacy set of the C extensions in
// pb_common.h.
#include "pb_atm_profile.h"
#include "pb_common.h"

namespace {

constexpr int kWave = 64;
using pb::atm::kBar;
constexpr double kEuler = 0.57721566490153286061;
constexpr double kE2Cutoff = 88.029691931113054296;   // log(2^127): E2 = 0 above, like the reference

// The LDS carve-up, in one place for the kernel and the launcher: four profile rows of
// lds_row(L) doubles (temperature, aux, mean mass, trapezoid), the VMR chunk [S][64], then
// PB_ATM_MAX_VMR powers of the Iso / Scale models.
__host__ __device__ inline int lds_row(int L) { return (L + 1) & ~1; }
__host__ __device__ inline size_t lds_doubles(int L, int S)
{
    return (size_t)4 * lds_row(L) + (size_t)S * kWave + PB_ATM_MAX_VMR;
}

struct AtmArgs {
    pb_atm_model m;
    const double *params;
    double *temps, *dens, *radius, *mm, *cdens, *adens;
    int32_t *reject;
    const int32_t *chem_status;   // [nw][L] of pb_equilibrium_vmr, or null
};

// Exponential integral E2(x), x >= 0, from its definitions (Abramowitz & Stegun 5.1.12, 5.1.22):
//   x <= 1: E2 = 1 - x (1 - gamma - ln x) - sum_{m >= 2} (-x)^m / ((m - 1) m!)   (24 terms: the
//           25th is below 1e-26)
//   x >  1: exp(-x) / (x + 2 - 1*2 / (x + 4 - 2*3 / (x + 6 - ...))), modified Lentz
__device__ double expint_e2(double x)
{
    if (x > kE2Cutoff)
        return 0.0;
    if (x == 0.0)
        return 1.0;
    if (x <= 1.0) {
        double term = -x;
        double sum = 0.0;
        for (int m = 2; m <= 24; m++) {
            term = term * (-x) / (double)m;
            sum += term / (double)(m - 1);
        }
        return (1.0 + (-x) * ((1.0 - kEuler) - log(x))) - sum;
    }
    double b = x + 2.0;
    double c = 1.0e300;
    double d = 1.0 / b;
    double h = d;
    for (int i = 1; i <= 400; i++) {
        const double an = -(double)i * (double)(i + 1);
        b += 2.0;
        d = 1.0 / (an * d + b);
        c = b + an / c;
        const double del = c * d;
        h *= del;
        if (fabs(del - 1.0) < 1.0e-16)
            break;
    }
    return h * exp(-x);
}

__device__ double guillot_xi(double gamma, double tau)
{
    const double gt = gamma * tau;
    return (2.0 / 3.0) * (((1.0 / gamma) * (1.0 + ((0.5 * gamma) * tau - 1.0) * exp(-gt)) +
                           (gamma * (1.0 - 0.5 * (tau * tau))) * expint_e2(gt)) + 1.0);
}

// np.sum(vmr * mass, axis=1) for one row of n <= 32 species (NumPy's pairwise sum below its block size:
// sequential under 8 elements, else 8 running sums combined as a tree, the remainder sequential)
__device__ double numpy_row_sum(const double *v, int stride, const double *mass, int n)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; i++)
            res += v[i * stride] * mass[i];
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; j++)
        r[j] = v[j * stride] * mass[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++)
            r[j] += v[(i + j) * stride] * mass[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++)
        res += v[i * stride] * mass[i];
    return res;
}

// The VMRs of layer l into column `lane` of s_vmr[nspecies][64]: the models, then the bulk balance.
// base_vmr: the walker's [nlayers][nspecies] (the shared one when base_vmr_stride is 0).
// Returns the mean molecular mass; *over_cap: the trace VMRs sum above qcap.
__device__ double layer_vmr(const pb_atm_model &m, const double *base_vmr, const double *par, int l,
                            int lane, double *s_vmr, const double *s_pow, unsigned bulk_mask,
                            bool *over_cap)
{
    const int S = m.nspecies;
    for (int sp = 0; sp < S; sp++)
        s_vmr[sp * kWave + lane] = base_vmr[(int64_t)l * S + sp];
    for (int i = 0; i < m.nvmr; i++) {
        const double *p = par + m.vmr_par[i];
        double v;
        if (m.vmr_kind[i] == 0) {
            v = s_pow[i];
        } else if (m.vmr_kind[i] == 1) {
            v = m.vmr0_d[(int64_t)i * m.nlayers + l] * s_pow[i];
        } else {
            double logv = p[0] * (m.log10p_d[l] - p[2]) + p[1];
            // np.clip = minimum(maximum(x, lo), hi)
            logv = logv < p[3] ? p[3] : logv;
            logv = logv > p[4] ? p[4] : logv;
            v = pow(10.0, logv);
        }
        s_vmr[m.vmr_species[i] * kWave + lane] = v;
    }
    // np.sum(vmr[:, ifree], axis=1), left to right: NumPy's own order below 8 trace species; from
    // 8 on NumPy sums pairwise and this sum can differ from it in the last bit
    double qtrace = 0.0;
    for (int sp = 0; sp < S; sp++)
        if (!((bulk_mask >> sp) & 1u))
            qtrace += s_vmr[sp * kWave + lane];
    *over_cap = m.has_qcap && qtrace > m.qcap;
    const double rest = 1.0 - qtrace;
    for (int j = 0; j < m.nbulk; j++)
        s_vmr[m.bulk_species[j] * kWave + lane] =
            (m.bulk_ratio_d[(int64_t)l * m.nbulk + j] * rest) * m.invsrat_d[l];
    return numpy_row_sum(s_vmr + lane, kWave, m.mass_d, S);
}

__device__ void gather_density(double *out, int64_t base, const int32_t *map, int ncol, int l0,
                               int nl, const double *s_vmr, const double *s_temp,
                               const double *pressure, bool rejected, int lane)
{
    // consecutive lanes write consecutive elements of out[walker][l0 .. l0 + nl)[ncol]
    for (int idx = lane; idx < nl * ncol; idx += kWave) {
        const int ll = idx / ncol, j = idx - ll * ncol;
        double v = 0.0;
        if (!rejected) {
            const int l = l0 + ll;
            v = pb::atm::ideal_gas_density(s_vmr[map[j] * kWave + ll], pressure[l], s_temp[l]);
        }
        out[base + (int64_t)l0 * ncol + idx] = v;
    }
}

// The walkers' T(p) (tmodels.py) into s_temp[L], s_aux[L] as work space (madhu's raw profile): one
// wavefront, the statements both k_walker_atmosphere and k_walker_temperature run (same bits).
// Returns the reject bits the model itself sets (madhu: log_p1 > log_p3).  The caller synchronises
// before it reads s_temp.
__device__ int walker_temperature(const pb_atm_model &m, const double *par, int lane, double *s_temp,
                                  double *s_aux)
{
    const int L = m.nlayers;
    const double *pressure = m.pressure_d;
    int flags = 0;
    if (m.tmodel == 0) {
        for (int l = lane; l < L; l += kWave)
            s_temp[l] = par[0];
    } else if (m.tmodel == 1) {
        const double kappa = pow(10.0, par[0]), gamma1 = pow(10.0, par[1]),
                     gamma2 = pow(10.0, par[2]);
        const double alpha = par[3];
        const double tirr4 = pow(par[4], 4.0), tint4 = pow(par[5], 4.0);
        for (int l = lane; l < L; l += kWave) {
            const double tau = kappa * (pressure[l] * kBar) / m.guillot_gravity;
            const double xi1 = guillot_xi(gamma1, tau), xi2 = guillot_xi(gamma2, tau);
            s_temp[l] = pow(0.75 * ((tint4 * (2.0 / 3.0 + tau) + (tirr4 * (1.0 - alpha)) * xi1) +
                                    (tirr4 * alpha) * xi2), 0.25);
        }
    } else {
        const double logp1 = par[0], logp2 = par[1], logp3 = par[2], a1 = par[3], a2 = par[4],
                     t0 = par[5];
        if (logp1 > logp3) {
            flags |= PB_ATM_REJECT_MADHU;
            for (int l = lane; l < L; l += kWave)
                s_temp[l] = 0.0;
        } else {
            const double d1 = a1 * m.madhu_loge, d2 = a2 * m.madhu_loge;
            const double q1 = (logp1 - m.madhu_logp0) / d1, q2 = (logp1 - logp2) / d2,
                         q3 = (logp3 - logp2) / d2;
            const double t1 = t0 + q1 * q1;
            const double t2 = t1 - q2 * q2;
            const double t3 = t2 + q3 * q3;
            for (int l = lane; l < L; l += kWave) {
                const double lp = m.log10p_d[l];
                double t;
                if (lp < logp1) {
                    const double q = (lp - m.madhu_logp0) / d1;
                    t = t0 + q * q;
                } else if (lp < logp3) {
                    const double q = (lp - logp2) / d2;
                    t = t2 + q * q;
                } else {
                    t = t3;
                }
                s_aux[l] = t;
            }
            __syncthreads();
            // scipy.ndimage.correlate1d with symmetric weights, mode='nearest': the centre tap,
            // then the pairs from the outermost inwards
            const int R = m.madhu_radius;
            const double *wt = m.madhu_weights_d;
            for (int l = lane; l < L; l += kWave) {
                double acc = s_aux[l] * wt[R];
                for (int k = -R; k < 0; k++) {
                    const int lo = max(l + k, 0), hi = min(l - k, L - 1);
                    acc += (s_aux[lo] + s_aux[hi]) * wt[k + R];
                }
                s_temp[l] = acc;
            }
        }
    }
    return flags;
}

__global__ __launch_bounds__(kWave) void k_walker_atmosphere(AtmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const pb_atm_model &m = a.m;
    const int L = m.nlayers, S = m.nspecies;
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x;
    const int Lp = lds_row(L);
    double *s_temp = reinterpret_cast<double *>(smem);   // temperatures
    double *s_aux = s_temp + Lp;                         // madhu's raw profile; integrand; radius
    double *s_mm = s_aux + Lp;                           // mean molecular mass
    double *s_int = s_mm + Lp;                           // cumulative trapezoid
    double *s_vmr = s_int + Lp;                          // [S][64] VMRs of a chunk of layers
    double *s_pow = s_vmr + S * kWave;                   // [nvmr] 10^p of the Iso / Scale models
    const double *par = a.params + w * m.npar;
    const double *pressure = m.pressure_d;
    const double *base_vmr = m.base_vmr_d + w * m.base_vmr_stride;
    int flags = 0;

    // ---- temperature (tmodels.py)
    flags |= walker_temperature(m, par, lane, s_temp, s_aux);
    for (int i = lane; i < m.nvmr; i += kWave)
        s_pow[i] = m.vmr_kind[i] == 2 ? 0.0 : pow(10.0, par[m.vmr_par[i]]);
    __syncthreads();
    for (int l = lane; l < L; l += kWave) {
        const double t = s_temp[l];
        if (!(t > 0.0) || !(fabs(t) <= 1.79769313486231570815e308))
            flags |= PB_ATM_REJECT_TEMP;
    }
    // Equilibrium chemistry: a cell that gave no VMRs rejects the walker (but PB_CHEM_REJECTED,
    // the temperature's own reject, flagged above).  Such a walker has no mean mass there, so its
    // radius is not judged (it is rejected already).
    bool no_vmr = false;
    if (a.chem_status) {
        bool missing = false;
        for (int l = lane; l < L; l += kWave) {
            const int32_t s = a.chem_status[w * L + l];
            missing = missing || s < 0;
            if (s < 0 && s != PB_CHEM_REJECTED)
                flags |= PB_ATM_REJECT_CHEMISTRY;
        }
        no_vmr = __any(missing) != 0;            // the block is one wavefront
    }

    // ---- abundances: the cap on the traces and the mean molecular mass of every layer
    unsigned bulk_mask = 0;
    for (int j = 0; j < m.nbulk; j++)
        bulk_mask |= 1u << m.bulk_species[j];
    for (int l = lane; l < L; l += kWave) {
        bool over;
        s_mm[l] = layer_vmr(m, base_vmr, par, l, lane, s_vmr, s_pow, bulk_mask, &over);
        if (over)
            flags |= PB_ATM_REJECT_QCAP;
    }

    // ---- hydrostatic radius (atmosphere.py:397-415, 467-485)
    const double mplanet = m.par_mplanet >= 0 ? par[m.par_mplanet] : m.mplanet;
    const double r0 = m.par_rplanet >= 0 ? par[m.par_rplanet] : m.rplanet;
    const double p0 = m.par_log_refpressure >= 0 ? pow(10.0, par[m.par_log_refpressure])
                                                 : m.refpressure;
    for (int l = lane; l < L; l += kWave)
        s_aux[l] = pb::atm::hydro_integrand(m.rmodel, s_temp[l], s_mm[l], mplanet, m.gplanet);
    __syncthreads();
    if (lane == 0)
        pb::atm::hydro_cumulative(s_int, m.lnp_d, s_aux, L);
    __syncthreads();
    if (!(p0 >= pressure[0] && p0 <= pressure[L - 1])) {
        flags |= PB_ATM_REJECT_REFPRESSURE;
    } else {
        const double i0 = pb::atm::hydro_reference(pressure, s_int, p0, L);
        for (int l = lane; l < L; l += kWave)
            s_aux[l] = pb::atm::hydro_radius(m.rmodel, s_int[l], i0, r0);
        __syncthreads();
        // a radius that is not finite and positive is no geometry for either model (a free
        // rplanet or mplanet that is NaN, zero or negative; every <= below is false on NaN)
        for (int l = lane; l < L; l += kWave)
            if (!no_vmr && (!(s_aux[l] > 0.0) || !(s_aux[l] <= 1.79769313486231570815e308)))
                flags |= PB_ATM_REJECT_DIVERGENT;
        if (m.rmodel == 0 && !no_vmr)
            for (int l = lane; l < L - 1; l += kWave)
                if (s_aux[l] <= s_aux[l + 1])
                    flags |= PB_ATM_REJECT_DIVERGENT;
    }
    for (int off = 1; off < kWave; off <<= 1)
        flags |= __shfl_xor(flags, off, kWave);
    const bool rejected = flags != 0;

    // ---- outputs, each written once
    if (lane == 0)
        a.reject[w] = flags;
    for (int l = lane; l < L; l += kWave) {
        a.temps[w * L + l] = rejected ? 0.0 : s_temp[l];
        a.mm[w * L + l] = rejected ? 0.0 : s_mm[l];
        a.radius[w * L + l] = rejected ? m.base_radius_d[l] : s_aux[l];
    }
    // s_vmr holds the full VMR of one chunk of 64 layers only (32 species x 1024 layers would not
    // fit in LDS), so the models and the bulk balance are evaluated a second time here, chunk by
    // chunk, on purpose: the first pass above kept only mm and the cap.  Same code, same bits.
    for (int l0 = 0; l0 < L; l0 += kWave) {
        const int nl = min(kWave, L - l0);
        __syncthreads();
        if (!rejected && lane < nl) {
            bool over;
            layer_vmr(m, base_vmr, par, l0 + lane, lane, s_vmr, s_pow, bulk_mask, &over);
        }
        __syncthreads();
        gather_density(a.dens, w * L * m.ntab, m.tab_map_d, m.ntab, l0, nl, s_vmr, s_temp,
                       pressure, rejected, lane);
        if (m.ncont)
            gather_density(a.cdens, w * L * m.ncont, m.cont_map_d, m.ncont, l0, nl, s_vmr, s_temp,
                           pressure, rejected, lane);
        if (m.nalk)
            gather_density(a.adens, w * L * m.nalk, m.alk_map_d, m.nalk, l0, nl, s_vmr, s_temp,
                           pressure, rejected, lane);
    }
}

// One wavefront per walker: the T(p) model alone, as formed (no reject contract).
__global__ __launch_bounds__(kWave) void k_walker_temperature(pb_atm_model m, const double *params,
                                                              double *temps)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int L = m.nlayers;
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x;
    double *s_temp = reinterpret_cast<double *>(smem);
    double *s_aux = s_temp + lds_row(L);
    walker_temperature(m, params + w * m.npar, lane, s_temp, s_aux);
    __syncthreads();
    for (int l = lane; l < L; l += kWave)
        temps[w * L + l] = s_temp[l];
}

inline int tmodel_npar(const pb_atm_model *m) { return m->tmodel == 0 ? 1 : 6; }

// What walker_temperature() needs of the struct, reported under the entry point's name `who`:
// the layers, the T(p) model, its parameter count, guillot's gravity, madhu's weights and the
// two arrays it reads.
int tmodel_check(const pb_atm_model *m, const char *who)
{
    PB_REQUIRE(m, "%s: null model struct", who);
    PB_REQUIRE(m->nlayers >= 2 && m->nlayers <= PB_ATM_MAX_LAYERS, "%s: 2-%d layers, not %d", who,
               PB_ATM_MAX_LAYERS, m->nlayers);
    PB_REQUIRE(m->tmodel >= 0 && m->tmodel <= 2,
               "%s: temperature model %d (0 isothermal, 1 guillot, 2 madhu)", who, m->tmodel);
    PB_REQUIRE(m->npar >= tmodel_npar(m), "%s: %d parameters, the temperature model takes %d", who,
               m->npar, tmodel_npar(m));
    if (m->tmodel == 1)
        PB_REQUIRE(m->guillot_gravity > 0.0, "%s: guillot gravity %g", who, m->guillot_gravity);
    if (m->tmodel == 2)
        PB_REQUIRE(m->madhu_radius >= 0 && m->madhu_weights_d && m->madhu_loge > 0.0,
                   "%s: madhu needs its smoothing weights (radius %d)", who, m->madhu_radius);
    PB_REQUIRE(m->pressure_d && m->log10p_d, "%s: null model array", who);
    return PB_OK;
}

// chem: the call of pb_walker_atmosphere_chem, which may come without bulk species
int atm_check(const pb_atm_model *m, bool chem)
{
    const int rc = tmodel_check(m, "pb_walker_atmosphere");
    if (rc != PB_OK)
        return rc;
    const int ntpar = tmodel_npar(m);
    PB_REQUIRE(m->nspecies >= 1 && m->nspecies <= PB_ATM_MAX_SPECIES,
               "pb_walker_atmosphere: 1-%d species, not %d", PB_ATM_MAX_SPECIES, m->nspecies);
    PB_REQUIRE(m->nvmr >= 0 && m->nvmr <= PB_ATM_MAX_VMR,
               "pb_walker_atmosphere: at most %d VMR models, not %d", PB_ATM_MAX_VMR, m->nvmr);
    PB_REQUIRE(m->nbulk >= (chem ? 0 : 1) && m->nbulk <= PB_ATM_MAX_BULK,
               "pb_walker_atmosphere: 1-%d bulk species, not %d", PB_ATM_MAX_BULK, m->nbulk);
    PB_REQUIRE(m->base_vmr_stride == 0 || m->base_vmr_stride == m->nlayers * m->nspecies,
               "pb_walker_atmosphere: base_vmr_stride %d (0: shared, or nlayers * nspecies = %d)",
               m->base_vmr_stride, m->nlayers * m->nspecies);
    unsigned used = 0;
    for (int j = 0; j < m->nbulk; j++) {
        PB_REQUIRE(m->bulk_species[j] >= 0 && m->bulk_species[j] < m->nspecies,
                   "pb_walker_atmosphere: bulk species %d of %d", m->bulk_species[j], m->nspecies);
        PB_REQUIRE(!((used >> m->bulk_species[j]) & 1u),
                   "pb_walker_atmosphere: bulk species %d listed twice", m->bulk_species[j]);
        used |= 1u << m->bulk_species[j];
    }
    bool scale = false;
    for (int i = 0; i < m->nvmr; i++) {
        PB_REQUIRE(m->vmr_kind[i] >= 0 && m->vmr_kind[i] <= 2,
                   "pb_walker_atmosphere: VMR model %d: kind %d", i, m->vmr_kind[i]);
        PB_REQUIRE(m->vmr_species[i] >= 0 && m->vmr_species[i] < m->nspecies,
                   "pb_walker_atmosphere: VMR model %d: species %d of %d", i, m->vmr_species[i],
                   m->nspecies);
        PB_REQUIRE(!((used >> m->vmr_species[i]) & 1u),
                   "pb_walker_atmosphere: VMR model %d: species %d is a bulk species or has a "
                   "model already", i, m->vmr_species[i]);
        used |= 1u << m->vmr_species[i];
        PB_REQUIRE(m->vmr_par[i] >= ntpar &&
                       m->vmr_par[i] + (m->vmr_kind[i] == 2 ? 5 : 1) <= m->npar,
                   "pb_walker_atmosphere: VMR model %d: parameters %d.. of %d", i, m->vmr_par[i],
                   m->npar);
        scale = scale || m->vmr_kind[i] == 1;
    }
    PB_REQUIRE(!scale || m->vmr0_d, "pb_walker_atmosphere: null vmr0 (ScaleVMR)");
    PB_REQUIRE((m->nbulk == 0 || (m->bulk_ratio_d && m->invsrat_d)) && m->base_vmr_d &&
                   m->lnp_d && m->mass_d && m->base_radius_d,
               "pb_walker_atmosphere: null model array");
    PB_REQUIRE(m->rmodel == 0 || m->rmodel == 1,
               "pb_walker_atmosphere: radius model %d (0 hydro_m, 1 hydro_g)", m->rmodel);
    const int free_par[3] = {m->par_rplanet, m->par_log_refpressure, m->par_mplanet};
    for (int j = 0; j < 3; j++)
        PB_REQUIRE(free_par[j] >= -1 && free_par[j] < m->npar,
                   "pb_walker_atmosphere: free scalar %d: column %d of %d", j, free_par[j], m->npar);
    PB_REQUIRE(m->par_rplanet < 0 || m->par_log_refpressure < 0,
               "pb_walker_atmosphere: rplanet and log_refpressure cannot both be free");
    PB_REQUIRE(m->par_rplanet >= 0 || m->rplanet > 0.0, "pb_walker_atmosphere: rplanet %g",
               m->rplanet);
    PB_REQUIRE(m->par_log_refpressure >= 0 || m->refpressure > 0.0,
               "pb_walker_atmosphere: refpressure %g", m->refpressure);
    if (m->rmodel == 0)
        PB_REQUIRE(m->par_mplanet >= 0 || m->mplanet > 0.0, "pb_walker_atmosphere: mplanet %g",
                   m->mplanet);
    else
        PB_REQUIRE(m->gplanet > 0.0, "pb_walker_atmosphere: gplanet %g", m->gplanet);
    PB_REQUIRE(m->ntab >= 1 && m->tab_map_d, "pb_walker_atmosphere: no table species (bind first)");
    PB_REQUIRE(m->ncont >= 0 && m->nalk >= 0 && (m->ncont == 0 || m->cont_map_d) &&
                   (m->nalk == 0 || m->alk_map_d),
               "pb_walker_atmosphere: bad continuum / alkali maps");
    return PB_OK;
}

int walker_atmosphere(const pb_atm_model *model, const double *params_d, int nwalkers,
                      const int32_t *chem_status_d, bool chem, double *temps_d, double *dens_d,
                      double *radius_d, double *mm_d, double *cont_dens_d, double *alk_dens_d,
                      int32_t *reject_d, void *stream)
{
    const int rc = atm_check(model, chem);
    if (rc != PB_OK)
        return rc;
    PB_REQUIRE(nwalkers >= 0, "pb_walker_atmosphere: %d walkers", nwalkers);
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(params_d && temps_d && dens_d && radius_d && mm_d && reject_d &&
                   (model->ncont == 0 || cont_dens_d) && (model->nalk == 0 || alk_dens_d),
               "pb_walker_atmosphere: null pointer");
    const size_t lds = sizeof(double) * lds_doubles(model->nlayers, model->nspecies);
    PB_REQUIRE(!chem || chem_status_d, "pb_walker_atmosphere_chem: null chem_status");
    AtmArgs a{*model, params_d, temps_d, dens_d, radius_d, mm_d, cont_dens_d, alk_dens_d, reject_d,
              chem_status_d};
    k_walker_atmosphere<<<nwalkers, kWave, lds, pb::as_stream(stream)>>>(a);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace

int pb_walker_atmosphere(const pb_atm_model *model, const double *params_d, int nwalkers,
                         double *temps_d, double *dens_d, double *radius_d, double *mm_d,
                         double *cont_dens_d, double *alk_dens_d, int32_t *reject_d, void *stream)
{
    return walker_atmosphere(model, params_d, nwalkers, nullptr, false, temps_d, dens_d, radius_d,
                             mm_d, cont_dens_d, alk_dens_d, reject_d, stream);
}

int pb_walker_atmosphere_chem(const pb_atm_model *model, const double *params_d, int nwalkers,
                              const int32_t *chem_status_d, double *temps_d, double *dens_d,
                              double *radius_d, double *mm_d, double *cont_dens_d,
                              double *alk_dens_d, int32_t *reject_d, void *stream)
{
    return walker_atmosphere(model, params_d, nwalkers, chem_status_d, true, temps_d, dens_d,
                             radius_d, mm_d, cont_dens_d, alk_dens_d, reject_d, stream);
}

int pb_walker_temperature(const pb_atm_model *model, const double *params_d, int nwalkers,
                          double *temps_d, void *stream)
{
    const int rc = tmodel_check(model, "pb_walker_temperature");
    if (rc != PB_OK)
        return rc;
    PB_REQUIRE(nwalkers >= 0, "pb_walker_temperature: %d walkers", nwalkers);
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(params_d && temps_d, "pb_walker_temperature: null pointer");
    const size_t lds = sizeof(double) * 2 * lds_row(model->nlayers);
    k_walker_temperature<<<nwalkers, kWave, lds, pb::as_stream(stream)>>>(*model, params_d,
                                                                          temps_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}
