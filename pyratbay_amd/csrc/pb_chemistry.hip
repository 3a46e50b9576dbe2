// pb_equilibrium_vmr: gas-phase thermochemical equilibrium of every (walker, layer) cell, one launch
// (what the reference asks chemcat for, pyratbay/pyrat/atmosphere.py:445-473; the statement of the
// arithmetic is ChemNetwork.equilibrium_host of pyratbay_amd/chemistry.py).
//
// One wavefront per cell, four cells per 256-thread block; lane i holds species i (its
// stoichiometry row, g_i, ln n_i), lanes >= S hold n = 0.  No LDS, no barriers, no atomics: every
// sum over species is one xor-butterfly reduction, after which all lanes hold the same bits, and
// every lane then solves the (E + 1) x (E + 1) system for itself.  The kernel is a template on E so
// that the matrix lives in compile-time-indexed registers (a runtime-indexed register array would go
// to scratch); the pivot row is found by compare-and-swap down the column for the same reason.
// Everything in binary64; the build's -ffp-contract=off keeps products and sums apart.
//
// pb_radeq_equilibrium is the same solver inside the radiative-equilibrium loop (pb_radeq.hip),
// where a cell's temperature moves by little between two launches: it starts from the iterate the
// previous launch left and also writes the mean molecular mass (k_radeq_equilibrium below).
//
// A network with ions and electrons (pb_chem_model.charge_d) adds the charge balance as one more
// row, the lane's charge as its balance column; both kernels are templates on (E, Charged), and the
// instantiations without charges are the kernels of a neutral network unchanged.  With charges the
// cold solve takes three steps (cold_solve_ions), all branches still uniform over the wavefront.
#include "pb_common.h"

namespace {

constexpr int kWave = 64;
constexpr int kCellsPerBlock = 4;
constexpr double kMinor = 1.0e-8;          // n_i / n at and below which a species is a minor one
constexpr double kLnMinor = 9.2103404;     // RP-1311 eq. 3.2: -ln(1e-4)
constexpr double kDblMax = 1.79769313486231570815e308;
constexpr double kTolIons = 1.0e-9;        // |dln n_i| of a charged species at convergence (TOL_ALL)

struct ChemArgs {
    pb_chem_model m;
    const double *temps, *params;
    double *vmr;
    int32_t *status;
    int64_t ncells;
};

// xor butterflies in a fixed order: lane and partner add the same two values, so every lane ends
// with the same bits
__device__ inline double wave_sum(double v)
{
    for (int off = kWave / 2; off >= 1; off >>= 1)
        v += __shfl_xor(v, off, kWave);
    return v;
}
__device__ inline double wave_max(double v)
{
    for (int off = kWave / 2; off >= 1; off >>= 1)
        v = fmax(v, __shfl_xor(v, off, kWave));
    return v;
}
__device__ inline double wave_min(double v)
{
    for (int off = kWave / 2; off >= 1; off >>= 1)
        v = fmin(v, __shfl_xor(v, off, kWave));
    return v;
}

// np.interp(x, xp[n], fp[0 : n * stride : stride]) for xp[0] <= x <= xp[n - 1] (the caller's check)
__device__ inline double interp_inside(const double *xp, const double *fp, int stride, int n,
                                       double x)
{
    int lo = 0, hi = n - 1;                    // largest lo with xp[lo] <= x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (xp[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    if (xp[hi] <= x)
        lo = hi;
    const double f0 = fp[(int64_t)lo * stride];
    if (lo == n - 1 || xp[lo] == x)
        return f0;
    const double slope = (fp[(int64_t)(lo + 1) * stride] - f0) / (xp[lo + 1] - xp[lo]);
    return slope * (x - xp[lo]) + f0;
}

// x of A x = r, in place (the solution in r): Gaussian elimination with partial pivoting, every
// index a compile-time constant
template <int N>
__device__ inline void gauss_solve(double (&A)[N][N], double (&r)[N])
{
#pragma unroll
    for (int k = 0; k < N; k++) {
#pragma unroll
        for (int i = k + 1; i < N; i++) {
            const bool swap = fabs(A[i][k]) > fabs(A[k][k]);
#pragma unroll
            for (int j = k; j < N; j++) {
                const double ai = A[i][j], ak = A[k][j];
                A[i][j] = swap ? ak : ai;
                A[k][j] = swap ? ai : ak;
            }
            const double ri = r[i], rk = r[k];
            r[i] = swap ? rk : ri;
            r[k] = swap ? ri : rk;
        }
#pragma unroll
        for (int i = k + 1; i < N; i++) {
            const double f = A[i][k] / A[k][k];
#pragma unroll
            for (int j = k + 1; j < N; j++)
                A[i][j] -= f * A[k][j];
            r[i] -= f * r[k];
        }
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double acc = r[i];
#pragma unroll
        for (int j = i + 1; j < N; j++)
            acc -= A[i][j] * r[j];
        r[i] = acc / A[i][i];
    }
}

// The two kernels below are made of the same two statements, each written once: the status of a
// cell before its iteration with its elemental abundances, and one Newton step.

// 0, or the PB_CHEM_* status of a cell that is not iterated; b[E] (zeros on entry): the elemental
// abundances of the walker whose parameters are par (ChemNetwork.element_abundances_host, the same
// statements)
template <int E>
__device__ __forceinline__ int cell_inputs(const pb_chem_model &m, const double *par, double t,
                                           double (&b)[E])
{
    int status = 0;
    if (!(t > 0.0))
        status = PB_CHEM_REJECTED;
    if (status == 0) {
        double dex[E];
        const double metal = m.par_metal >= 0 ? par[m.par_metal] : 0.0;
#pragma unroll
        for (int j = 0; j < E; j++)
            dex[j] = m.is_metal[j] ? m.base_dex[j] + metal : m.base_dex[j];
        for (int k = 0; k < m.nscale; k++) {
            const double v = par[m.scale_par[k]];
#pragma unroll
            for (int j = 0; j < E; j++)
                if (m.scale_element[k] == j)
                    dex[j] = m.base_dex[j] + v;
        }
        bool bad = false;
        for (int k = 0; k < m.nratio; k++) {
            const double v = par[m.ratio_par[k]];
            if (!(v > 0.0))
                bad = true;
            double den = 0.0;
#pragma unroll
            for (int j = 0; j < E; j++)
                if (m.ratio_den[k] == j)
                    den = dex[j];
            const double num = den + log10(v);
#pragma unroll
            for (int j = 0; j < E; j++)
                if (m.ratio_num[k] == j)
                    dex[j] = num;
        }
        double dex_h = 0.0;
#pragma unroll
        for (int j = 0; j < E; j++)
            if (m.ihydrogen == j)
                dex_h = dex[j];
#pragma unroll
        for (int j = 0; j < E; j++) {
            b[j] = pow(10.0, dex[j] - dex_h);
            if (!(b[j] > 0.0) || !(b[j] <= kDblMax))
                bad = true;
        }
        if (bad)
            status = PB_CHEM_RATIO;
    }
    if (status == 0 && !(t >= m.gibbs_temps_d[0] && t <= m.gibbs_temps_d[m.ntemps - 1]))
        status = PB_CHEM_TEMPERATURE;
    return status;
}

// One iteration on this lane's ln_ni and the cell's ln_n, both updated; returns the convergence
// test of pb_equilibrium_vmr (a full step, weighed by n_i).  dln_ni: this lane's undamped step
// (0 in a lane without a species), which that test does not bound for a trace species.  pi: the
// potentials of this solve.
// Charged: the last balance column is the lane's charge and b's last entry 0, so the system has
// order E + 1 with E counting that row.  The weighted test does not see a trace species, hence not
// the charge balance: a charged lane also needs |dln n_i| < kTolIons.  sum_i q_i^2 n_i == 0 (every
// ion has underflowed; the same bits in all lanes): an identity row in place of the charge row and
// column, and the charged lanes keep their ln n_i for this step.
template <int E, bool Charged = false>
__device__ __forceinline__ bool newton_step(const pb_chem_model &m, bool live,
                                            const double (&stoich)[E], const double (&b)[E],
                                            double g, double lnp, double &ln_ni, double &ln_n,
                                            double &dln_ni, double (&pi)[E])
{
    constexpr int N = E + 1;
    const double ni = live ? exp(ln_ni) : 0.0;
    const double n = exp(ln_n);
    const double mu = live ? ((g + ln_ni) - ln_n) + lnp : 0.0;
    double an[E];
#pragma unroll
    for (int k = 0; k < E; k++)
        an[k] = stoich[k] * ni;
    double A[N][N], r[N];
#pragma unroll
    for (int k = 0; k < E; k++) {
#pragma unroll
        for (int j = k; j < E; j++) {
            const double s = wave_sum(stoich[k] * an[j]);
            A[k][j] = s;
            A[j][k] = s;
        }
        const double col = wave_sum(an[k]);
        A[k][E] = col;
        A[E][k] = col;
        r[k] = (b[k] - col) + wave_sum(an[k] * mu);
    }
    const double sn = wave_sum(ni);
    A[E][E] = sn - n;
    r[E] = (n - sn) + wave_sum(ni * mu);
    if constexpr (Charged) {
        const bool drop = A[E - 1][E - 1] == 0.0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            A[E - 1][j] = drop ? 0.0 : A[E - 1][j];
            A[j][E - 1] = drop ? 0.0 : A[j][E - 1];
        }
        A[E - 1][E - 1] = drop ? 1.0 : A[E - 1][E - 1];
        r[E - 1] = drop ? 0.0 : r[E - 1];
        live = live && !(drop && stoich[E - 1] != 0.0);
    }
    gauss_solve<N>(A, r);
    const double dln_n = r[E];
    double api = 0.0;
#pragma unroll
    for (int j = 0; j < E; j++) {
        api += stoich[j] * r[j];
        pi[j] = r[j];
    }
    dln_ni = live ? (-mu + dln_n) + api : 0.0;

    // ---- damping (RP-1311 eqs. 3.1-3.3)
    const bool major = live && ni / n > kMinor;
    const double step = wave_max(major ? fabs(dln_ni) : 0.0);
    const double l1 = 2.0 / fmax(5.0 * fabs(dln_n), step);
    const bool minor = live && !major && dln_ni >= 0.0;
    const double q = minor ? fabs((-(ln_ni - ln_n) - kLnMinor) / (dln_ni - dln_n)) : INFINITY;
    const double l2 = wave_min(q);
    const double lambda = fmin(1.0, fmin(l1, l2));
    ln_ni += lambda * dln_ni;
    ln_n += lambda * dln_n;
    // n_i |dln n_i| / sum n < tolerance in every lane (false on NaN, like the host's)
    const bool open = live && !((ni * fabs(dln_ni)) / sn < m.tolerance);
    if constexpr (Charged)
        if (__any(live && stoich[E - 1] != 0.0 && !(fabs(dln_ni) < kTolIons)))
            return false;
    return lambda == 1.0 && !__any(open) && fabs(dln_n) < m.tolerance;
}

// A lane's balance row [stoich | charge] and the right-hand side [b | 0] of the charged system
template <int E>
__device__ __forceinline__ void with_charge(const double (&stoich)[E], const double (&b)[E],
                                            double charge, double (&bal)[E + 1],
                                            double (&b0)[E + 1])
{
#pragma unroll
    for (int j = 0; j < E; j++) {
        bal[j] = stoich[j];
        b0[j] = b[j];
    }
    bal[E] = charge;
    b0[E] = 0.0;
}

// The cold solve of a cell whose network has charged species (ChemNetwork._cold_ions, the same
// statements), in three steps.  From the cold start the ions would approach their values by one
// unit of ln n per iteration (Newton on e^u - e^v = 0), dG_ion / (2 R T) iterations, so:
//   1. the neutral lanes alone, from the cold start of their sub-network: its statements and bits;
//   2. the charged lanes seeded from its potentials: ln n_i = t_i + q_i pi_q with
//      t_i = ln n - g_i - ln p + sum_j a_ij pi_j and pi_q = (LSE- - LSE+) / 2, the log-sum-exp of t
//      over the lanes of either sign (two wave maxima, two wave sums): exact for charges +-1 while
//      the ions are trace, and never underflowing;
//   3. the full system of order E + 2 from there.
// Each loop is capped at max_iterations; iterations: their sum.  Returns whether both converged.
template <int E>
__device__ __forceinline__ bool cold_solve_ions(const pb_chem_model &m, bool live, double charge,
                                                const double (&stoich)[E], const double (&b)[E],
                                                double g, double lnp, double &ln_ni,
                                                double &ln_n, int &iterations)
{
    const bool neutral = live && charge == 0.0;
    const int count = __popcll(__ballot(neutral));
    ln_ni = neutral ? log(0.1 / (double)count) : 0.0;
    ln_n = log(0.1);
    double dln_ni, pi[E];
    bool converged = false;
    iterations = 0;
    for (int it = 1; it <= m.max_iterations && !converged; it++) {
        converged = newton_step<E>(m, neutral, stoich, b, g, lnp, ln_ni, ln_n, dln_ni, pi);
        iterations = it;
    }
    if (!converged)
        return false;

    double api = 0.0;
#pragma unroll
    for (int j = 0; j < E; j++)
        api += stoich[j] * pi[j];
    const double t = ((ln_n - g) - lnp) + api;
    const bool minus = live && charge < 0.0, plus = live && charge > 0.0;
    const double top_minus = wave_max(minus ? t : -INFINITY);
    const double top_plus = wave_max(plus ? t : -INFINITY);
    const double lse_minus = top_minus + log(wave_sum(minus ? exp(t - top_minus) : 0.0));
    const double lse_plus = top_plus + log(wave_sum(plus ? exp(t - top_plus) : 0.0));
    const double pi_q = 0.5 * (lse_minus - lse_plus);
    if (minus || plus)
        ln_ni = t + charge * pi_q;

    double bal[E + 1], b0[E + 1], pi0[E + 1];
    with_charge<E>(stoich, b, charge, bal, b0);
    const int first = iterations;
    converged = false;
    for (int it = 1; it <= m.max_iterations && !converged; it++) {
        converged = newton_step<E + 1, true>(m, live, bal, b0, g, lnp, ln_ni, ln_n, dln_ni, pi0);
        iterations = first + it;
    }
    return converged;
}

// Charged: the network has ions and electrons (m.charge_d), E < PB_CHEM_MAX_ELEMENTS; without, the
// kernel is that of a neutral network to the instruction.
template <int E, bool Charged>
__global__ __launch_bounds__(kWave * kCellsPerBlock) void k_equilibrium_vmr(ChemArgs a)
{
    const pb_chem_model &m = a.m;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t cell = (int64_t)blockIdx.x * kCellsPerBlock + (threadIdx.x >> 6);
    if (cell >= a.ncells)                      // a whole wavefront: the kernel has no barrier
        return;
    const int S = m.nspecies, L = m.nlayers;
    const int64_t w = cell / L;
    const int l = (int)(cell - w * L);
    const bool live = lane < S;
    const double *par = a.params + w * m.npar;   // dereferenced only at a column >= 0 (the check)
    const double t = a.temps[cell];

    double b[E] = {};
    int status = cell_inputs<E>(m, par, t, b);

    double x = 0.0;                            // this lane's VMR
    double stoich[E];
#pragma unroll
    for (int j = 0; j < E; j++)
        stoich[j] = live ? (double)m.stoich_d[lane * E + j] : 0.0;

    if (status == 0) {
        const double g = live ? interp_inside(m.gibbs_temps_d, m.gibbs_d + lane, S, m.ntemps, t)
                              : 0.0;
        const double lnp = log(m.pressure_d[l]);
        double ln_ni = live ? log(0.1 / (double)S) : 0.0;
        double ln_n = log(0.1);
        int iterations = 0;
        bool converged = false;
        if constexpr (Charged) {
            const double charge = live ? (double)m.charge_d[lane] : 0.0;
            converged = cold_solve_ions<E>(m, live, charge, stoich, b, g, lnp, ln_ni, ln_n,
                                           iterations);
        } else {
            for (int it = 1; it <= m.max_iterations && !converged; it++) {
                double dln_ni, pi[E];
                converged = newton_step<E>(m, live, stoich, b, g, lnp, ln_ni, ln_n, dln_ni, pi);
                iterations = it;
            }
        }
        if (converged) {
            const double ni = live ? exp(ln_ni) : 0.0;
            x = ni / wave_sum(ni);
            status = iterations;
        } else {
            status = PB_CHEM_NOT_CONVERGED;
        }
    }

    // ---- hybrid models: free log10(VMR)s on top of the equilibrium, capped by the elements the
    // equilibrium mixture holds (vmr_models.py:40-57); nothing is renormalised
    if (status > 0 && m.nhybrid > 0) {
        double total[E];
#pragma unroll
        for (int j = 0; j < E; j++)
            total[j] = wave_sum(x * stoich[j]);
        double out = x;
        for (int k = 0; k < m.nhybrid; k++) {
            const int sp = m.hybrid_species[k];
            double cap = INFINITY;
#pragma unroll
            for (int j = 0; j < E; j++) {
                const int sj = m.stoich_d[sp * E + j];
                if (sj > 0) {
                    const double c = total[j] / (double)sj;
                    cap = c < cap ? c : cap;
                }
            }
            // np.clip = minimum(maximum(v, 0), cap)
            double v = pow(10.0, par[m.hybrid_par[k]]);
            v = v < 0.0 ? 0.0 : v;
            v = v > cap ? cap : v;
            if (lane == sp)
                out = v;
        }
        x = out;
    }

    // ---- outputs, each written once
    if (live)
        a.vmr[cell * S + lane] = status > 0 ? x : 0.0;
    if (lane == 0)
        a.status[cell] = status;
}

// ------------------------------------------------------- pb_radeq_equilibrium: a carried iterate

struct CarriedArgs {
    pb_chem_model m;
    pb_radeq_chem c;
    const double *temps, *params;
    int64_t ncells;
    int warm;
};

// k_equilibrium_vmr (the same layout, no hybrid models) inside the radiative-equilibrium loop: the
// iterate of every cell is kept in c.ln_ni_d, c.ln_n_d from launch to launch.  warm == 0: the cold
// start and the test of k_equilibrium_vmr, hence its bits.  warm != 0: from the stored iterate,
// converged when that test holds AND |dln n_i| < tol_all in every lane with a species (the test
// alone passes a trace species after one step from a converged neighbour state; the step of a
// trace species then still carries the first-order error of the major ones); a stored iterate
// that is not finite, or max_iterations without convergence, and the cell is solved from the cold
// start as with warm == 0.  Every branch on these is uniform over the wavefront: the values come
// out of butterflies and ballots.  A cell that ends with a negative status leaves vmr_d, mm_d and
// its iterate as they were and counts in failures_d, which only its own lane 0 writes.
// Charged: a carried iterate goes straight to the full system with the charge row (step 3 of
// cold_solve_ions, with both tests and that of the charged lanes), the cold solve is the three
// steps; the mean mass counts the electrons through the caller's mol_mass_d.
template <int E, bool Charged>
__global__ __launch_bounds__(kWave * kCellsPerBlock) void k_radeq_equilibrium(CarriedArgs a)
{
    const pb_chem_model &m = a.m;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t cell = (int64_t)blockIdx.x * kCellsPerBlock + (threadIdx.x >> 6);
    if (cell >= a.ncells)                      // a whole wavefront: the kernel has no barrier
        return;
    const int S = m.nspecies, L = m.nlayers;
    const int64_t w = cell / L;
    const int l = (int)(cell - w * L);
    const bool live = lane < S;
    const double *par = a.params + w * m.npar;   // dereferenced only at a column >= 0 (the check)
    const double t = a.temps[cell];

    double b[E] = {};
    int status = cell_inputs<E>(m, par, t, b);

    double x = 0.0;                            // this lane's VMR
    double ln_ni = 0.0, ln_n = 0.0;
    double stoich[E];
#pragma unroll
    for (int j = 0; j < E; j++)
        stoich[j] = live ? (double)m.stoich_d[lane * E + j] : 0.0;

    if (status == 0) {
        const double g = live ? interp_inside(m.gibbs_temps_d, m.gibbs_d + lane, S, m.ntemps, t)
                              : 0.0;
        const double lnp = log(m.pressure_d[l]);
        bool carried = false;
        if (a.warm) {
            ln_ni = live ? a.c.ln_ni_d[cell * S + lane] : 0.0;
            ln_n = a.c.ln_n_d[cell];
            carried = !__any(!(fabs(ln_ni) <= kDblMax)) && fabs(ln_n) <= kDblMax;
        }
        int iterations = 0;
        bool converged = false;
        if constexpr (Charged) {
            // a carried iterate goes straight to the full system; the cold solve is the three
            // steps of cold_solve_ions
            const double charge = live ? (double)m.charge_d[lane] : 0.0;
            if (carried) {
                double bal[E + 1], b0[E + 1];
                with_charge<E>(stoich, b, charge, bal, b0);
                for (int it = 1; it <= m.max_iterations && !converged; it++) {
                    double dln_ni, pi[E + 1];
                    converged = newton_step<E + 1, true>(m, live, bal, b0, g, lnp, ln_ni, ln_n,
                                                         dln_ni, pi);
                    if (__any(!(fabs(dln_ni) < a.c.tol_all)))
                        converged = false;
                    iterations = it;
                }
            }
            if (!converged)
                converged = cold_solve_ions<E>(m, live, charge, stoich, b, g, lnp, ln_ni, ln_n,
                                               iterations);
        } else {
            for (;;) {
                if (!carried) {
                    ln_ni = live ? log(0.1 / (double)S) : 0.0;
                    ln_n = log(0.1);
                }
                for (int it = 1; it <= m.max_iterations && !converged; it++) {
                    double dln_ni, pi[E];
                    converged = newton_step<E>(m, live, stoich, b, g, lnp, ln_ni, ln_n, dln_ni,
                                               pi);
                    if (carried && __any(!(fabs(dln_ni) < a.c.tol_all)))
                        converged = false;
                    iterations = it;
                }
                if (converged || !carried)
                    break;
                carried = false;
            }
        }
        if (converged) {
            const double ni = live ? exp(ln_ni) : 0.0;
            x = ni / wave_sum(ni);
            status = iterations;
        } else {
            status = PB_CHEM_NOT_CONVERGED;
        }
    }

    // ---- outputs, each written once; nothing but the status of a cell without a solution
    if (status > 0) {
        const double mm = wave_sum(live ? x * a.c.mol_mass_d[lane] : 0.0);
        if (live) {
            a.c.vmr_d[cell * S + lane] = x;
            a.c.ln_ni_d[cell * S + lane] = ln_ni;
        }
        if (lane == 0) {
            a.c.mm_d[cell] = mm;
            a.c.ln_n_d[cell] = ln_n;
        }
    }
    if (lane == 0) {
        a.c.status_d[cell] = status;
        if (status < 0)
            a.c.failures_d[cell] += 1;
    }
}

int chem_check(const pb_chem_model *m, const char *name)
{
    PB_REQUIRE(m, "%s: null model struct", name);
    PB_REQUIRE(m->nspecies >= 1 && m->nspecies <= PB_CHEM_MAX_SPECIES,
               "%s: 1-%d species, not %d", name, PB_CHEM_MAX_SPECIES, m->nspecies);
    PB_REQUIRE(m->nelements >= 1 && m->nelements <= PB_CHEM_MAX_ELEMENTS,
               "%s: 1-%d elements, not %d", name, PB_CHEM_MAX_ELEMENTS, m->nelements);
    PB_REQUIRE(!m->charge_d || m->nelements + 1 <= PB_CHEM_MAX_ELEMENTS,
               "%s: %d elements with charges: the charge balance takes one of the %d rows", name,
               m->nelements, PB_CHEM_MAX_ELEMENTS);
    PB_REQUIRE(m->ntemps >= 1, "%s: %d Gibbs temperatures", name, m->ntemps);
    PB_REQUIRE(m->nlayers >= 1, "%s: %d layers", name, m->nlayers);
    PB_REQUIRE(m->npar >= 0, "%s: %d parameters", name, m->npar);
    PB_REQUIRE(m->ihydrogen >= 0 && m->ihydrogen < m->nelements,
               "%s: hydrogen is element %d of %d", name, m->ihydrogen, m->nelements);
    PB_REQUIRE(m->par_metal >= -1 && m->par_metal < m->npar,
               "%s: [M/H] in column %d of %d", name, m->par_metal, m->npar);
    PB_REQUIRE(m->nscale >= 0 && m->nscale <= PB_CHEM_MAX_ELEMENTS,
               "%s: at most %d [X/H], not %d", name, PB_CHEM_MAX_ELEMENTS, m->nscale);
    for (int k = 0; k < m->nscale; k++)
        PB_REQUIRE(m->scale_element[k] >= 0 && m->scale_element[k] < m->nelements &&
                       m->scale_par[k] >= 0 && m->scale_par[k] < m->npar,
                   "%s: [X/H] %d: element %d of %d, column %d of %d", name, k,
                   m->scale_element[k], m->nelements, m->scale_par[k], m->npar);
    PB_REQUIRE(m->nratio >= 0 && m->nratio <= PB_CHEM_MAX_ELEMENTS,
               "%s: at most %d X/Y, not %d", name, PB_CHEM_MAX_ELEMENTS, m->nratio);
    for (int k = 0; k < m->nratio; k++)
        PB_REQUIRE(m->ratio_num[k] >= 0 && m->ratio_num[k] < m->nelements &&
                       m->ratio_den[k] >= 0 && m->ratio_den[k] < m->nelements &&
                       m->ratio_par[k] >= 0 && m->ratio_par[k] < m->npar,
                   "%s: X/Y %d: elements %d and %d of %d, column %d of %d", name, k,
                   m->ratio_num[k], m->ratio_den[k], m->nelements, m->ratio_par[k], m->npar);
    PB_REQUIRE(m->nhybrid >= 0 && m->nhybrid <= PB_CHEM_MAX_HYBRID,
               "%s: at most %d hybrid models, not %d", name, PB_CHEM_MAX_HYBRID,
               m->nhybrid);
    for (int k = 0; k < m->nhybrid; k++)
        PB_REQUIRE(m->hybrid_species[k] >= 0 && m->hybrid_species[k] < m->nspecies &&
                       m->hybrid_par[k] >= 0 && m->hybrid_par[k] < m->npar,
                   "%s: hybrid model %d: species %d of %d, column %d of %d", name, k,
                   m->hybrid_species[k], m->nspecies, m->hybrid_par[k], m->npar);
    PB_REQUIRE(m->max_iterations >= 1 && m->max_iterations <= 10000,
               "%s: max_iterations %d (1-10000)", name, m->max_iterations);
    PB_REQUIRE(m->tolerance > 0.0, "%s: tolerance %g", name, m->tolerance);
    PB_REQUIRE(m->gibbs_temps_d && m->gibbs_d && m->stoich_d && m->pressure_d,
               "%s: null model array", name);
    return PB_OK;
}

template <int E, bool Charged>
void launch(const ChemArgs &a, unsigned blocks, hipStream_t stream)
{
    k_equilibrium_vmr<E, Charged><<<blocks, kWave * kCellsPerBlock, 0, stream>>>(a);
}
template <int E, bool Charged>
void launch(const CarriedArgs &a, unsigned blocks, hipStream_t stream)
{
    k_radeq_equilibrium<E, Charged><<<blocks, kWave * kCellsPerBlock, 0, stream>>>(a);
}

// the instantiation of a model: its elements, and whether it has charges (chem_check: then at
// most PB_CHEM_MAX_ELEMENTS - 1 elements)
template <class Args>
void launch_model(const Args &a, unsigned blocks, hipStream_t stream)
{
    if (a.m.charge_d) {
        switch (a.m.nelements) {
        case 1: launch<1, true>(a, blocks, stream); break;
        case 2: launch<2, true>(a, blocks, stream); break;
        case 3: launch<3, true>(a, blocks, stream); break;
        case 4: launch<4, true>(a, blocks, stream); break;
        case 5: launch<5, true>(a, blocks, stream); break;
        case 6: launch<6, true>(a, blocks, stream); break;
        default: launch<7, true>(a, blocks, stream); break;
        }
        return;
    }
    switch (a.m.nelements) {
    case 1: launch<1, false>(a, blocks, stream); break;
    case 2: launch<2, false>(a, blocks, stream); break;
    case 3: launch<3, false>(a, blocks, stream); break;
    case 4: launch<4, false>(a, blocks, stream); break;
    case 5: launch<5, false>(a, blocks, stream); break;
    case 6: launch<6, false>(a, blocks, stream); break;
    case 7: launch<7, false>(a, blocks, stream); break;
    default: launch<8, false>(a, blocks, stream); break;
    }
}

}  // namespace

int pb_radeq_equilibrium(const pb_chem_model *model, const double *temps_d,
                         const double *params_d, int nwalkers, int warm,
                         const pb_radeq_chem *state, void *stream)
{
    const int rc = chem_check(model, "pb_radeq_equilibrium");
    if (rc != PB_OK)
        return rc;
    PB_REQUIRE(model->nhybrid == 0, "pb_radeq_equilibrium: %d hybrid models: the carried iterate "
               "is that of the equilibrium alone", model->nhybrid);
    PB_REQUIRE(nwalkers >= 0, "pb_radeq_equilibrium: %d walkers", nwalkers);
    PB_REQUIRE(state, "pb_radeq_equilibrium: null state struct");
    if (nwalkers == 0)
        return PB_OK;
    const pb_radeq_chem &c = *state;
    PB_REQUIRE(temps_d && c.ln_ni_d && c.ln_n_d && c.vmr_d && c.mm_d && c.mol_mass_d &&
                   c.status_d && c.failures_d,
               "pb_radeq_equilibrium: null pointer");
    PB_REQUIRE(params_d || model->npar == 0, "pb_radeq_equilibrium: null params with %d columns",
               model->npar);
    PB_REQUIRE(c.tol_all > 0.0, "pb_radeq_equilibrium: tol_all %g", c.tol_all);
    const int64_t ncells = (int64_t)nwalkers * model->nlayers;
    const int64_t blocks = (ncells + kCellsPerBlock - 1) / kCellsPerBlock;
    PB_REQUIRE(blocks <= 0x7fffffffLL, "pb_radeq_equilibrium: %lld cells are too many for one "
               "launch", (long long)ncells);
    CarriedArgs a{*model, c, temps_d, params_d, ncells, warm};
    launch_model(a, (unsigned)blocks, pb::as_stream(stream));
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_equilibrium_vmr(const pb_chem_model *model, const double *temps_d, const double *params_d,
                       int nwalkers, double *vmr_d, int32_t *status_d, void *stream)
{
    const int rc = chem_check(model, "pb_equilibrium_vmr");
    if (rc != PB_OK)
        return rc;
    PB_REQUIRE(nwalkers >= 0, "pb_equilibrium_vmr: %d walkers", nwalkers);
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(temps_d && vmr_d && status_d, "pb_equilibrium_vmr: null pointer");
    PB_REQUIRE(params_d || model->npar == 0, "pb_equilibrium_vmr: null params with %d columns",
               model->npar);
    const int64_t ncells = (int64_t)nwalkers * model->nlayers;
    const int64_t blocks = (ncells + kCellsPerBlock - 1) / kCellsPerBlock;
    PB_REQUIRE(blocks <= 0x7fffffffLL, "pb_equilibrium_vmr: %lld cells are too many for one launch",
               (long long)ncells);
    ChemArgs a{*model, temps_d, params_d, vmr_d, status_d, ncells};
    launch_model(a, (unsigned)blocks, pb::as_stream(stream));
    PB_LAUNCH_CHECK();
    return PB_OK;
}
