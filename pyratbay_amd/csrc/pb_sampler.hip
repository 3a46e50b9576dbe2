// The sampler of the batched retrieval loop: DEMC-zs (ter Braak & Vrugt 2008, Stat. Comput. 18,
// 435), many parallel chains whose proposals are differences of rows of a shared history, so that
// one generation is one batch: k_demc_propose -> the caller's log-posterior -> k_demc_accept.  The
// NumPy statements of pyratbay_amd/sampler.py (propose_host, accept_host, gelman_rubin_host,
// uniforms_host) are the specification; pb_philox.h gives both sides the same random words.
//
// One wavefront per chain, the free parameters two per lane (lane and lane + 64, as
// k_retrieval_map); every dot product is summed in a fixed order (the lane's two terms, then a
// butterfly).  No scratch, no atomics; the generation, the history's length and the flags travel
// by value.  Plain launches: no allocation, no synchronisation.
#include "pb_common.h"
#include "pb_philox.h"

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kMaxPar = PB_RETRIEVAL_MAX_PARAMS;
static_assert(kMaxPar == 2 * kWave, "the sampler's kernels give every lane two parameters");

// the normal of parameter f: Box-Muller on block 3 + f / 2, cosine for even f, sine for odd f
__device__ __forceinline__ double normal_of(uint64_t seed, uint32_t w, uint32_t g, int f)
{
    double ua, ub;
    pb::philox_block_uniforms(seed, 3u + (uint32_t)(f >> 1), w, g, pb::kTagPropose, ua, ub);
    const double r = sqrt(-2.0 * log(ua));
    const double angle = (2.0 * pb::kPi) * ub;
    return r * ((f & 1) ? sin(angle) : cos(angle));
}

__global__ __launch_bounds__(kWave * kWavesPerBlock) void k_demc_propose(
    double *__restrict__ prop, double *__restrict__ log_jac, int32_t *__restrict__ kind,
    const double *__restrict__ theta, const double *__restrict__ z,
    const double *__restrict__ pstep, uint32_t g, uint64_t seed, int64_t M, double gamma,
    double fepsilon, double p_snooker, int nfree, int nw)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int w = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (w >= nw)                                        // (wave-uniform)
        return;
    double ua, ub, us, ug;
    pb::philox_block_uniforms(seed, 0u, (uint32_t)w, g, pb::kTagPropose, ua, ub);
    const int64_t r1 = pb::philox_index(ua, M);
    int64_t r2 = pb::philox_index(ub, M - 1);
    r2 += (r2 >= r1) ? 1 : 0;
    pb::philox_block_uniforms(seed, 1u, (uint32_t)w, g, pb::kTagPropose, us, ub);
    const int64_t rz = pb::philox_index(ub, M);
    pb::philox_block_uniforms(seed, 2u, (uint32_t)w, g, pb::kTagPropose, ug, ub);
    const bool snooker = us < p_snooker;                // (wave-uniform)

    const double *row = theta + (int64_t)w * nfree;
    const double *z1 = z + r1 * nfree, *z2 = z + r2 * nfree, *zr = z + rz * nfree;
    double *out = prop + (int64_t)w * nfree;
    if (!snooker) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int f = lane + h * kWave;
            if (f < nfree) {
                const double n = normal_of(seed, (uint32_t)w, g, f);
                const double jump = row[f] + gamma * (z1[f] - z2[f]);
                out[f] = jump + (fepsilon * pstep[f]) * n;
            }
        }
        if (lane == 0) {
            log_jac[w] = 0.0;
            kind[w] = 0;
        }
        return;
    }
    // the snooker update: a jump along the line through the chain and Z[rz], its length from the
    // projection of Z[r1] - Z[r2] on that line
    double th[2] = {0.0, 0.0}, d[2] = {0.0, 0.0}, anchor[2] = {0.0, 0.0};
    double dd = 0.0, pd = 0.0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int f = lane + h * kWave;
        if (f < nfree) {
            th[h] = row[f];
            anchor[h] = zr[f];
            d[h] = th[h] - anchor[h];
            dd += d[h] * d[h];
            pd += (z1[f] - z2[f]) * d[h];
        }
    }
    const double D2 = pb::wave_sum(dd);
    const double proj = pb::wave_sum(pd);
    const double c = (1.2 + ug) * (proj / D2);
    double p[2], ee = 0.0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        p[h] = th[h] + c * d[h];
        const double e = p[h] - anchor[h];
        ee += (lane + h * kWave < nfree) ? e * e : 0.0;
    }
    const double N2 = pb::wave_sum(ee);
    double lj = (0.5 * (double)(nfree - 1)) * (log(N2) - log(D2));
    const bool ok = D2 > 0.0 && isfinite(lj);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int f = lane + h * kWave;
        if (f < nfree)
            out[f] = ok ? p[h] : th[h];
    }
    if (lane == 0) {
        log_jac[w] = ok ? lj : 0.0;
        kind[w] = 1;
    }
}

struct AcceptArgs {
    double *theta, *logp;                       // [nw, nfree], [nw]: in place
    const double *prop, *logp_prop, *log_jac;
    double *rows, *row_logp;                    // [nw, cap, nfree], [nw, cap]
    int32_t *row_gen;                           // [nw, cap]
    int64_t *counts;                            // [nw, cap]
    int32_t *nrows, *overflow;                  // [nw]
    double *mean, *m2;                          // [nw, nfree]
    int64_t *nstat;                             // [nw]
    double *z;                                  // [Mcap, nfree]
    int32_t *accepted;                          // [nw]
    uint64_t seed;
    int64_t M;
    uint32_t g;
    int append, cap, nfree, nw;
};

__global__ __launch_bounds__(kWave * kWavesPerBlock) void k_demc_accept(AcceptArgs a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int w = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (w >= a.nw)                                      // (wave-uniform)
        return;
    double u, unused;
    pb::philox_block_uniforms(a.seed, 0u, (uint32_t)w, a.g, pb::kTagAccept, u, unused);
    const double lp = a.logp[w], lpp = a.logp_prop[w], lj = a.log_jac[w];
    // (a NaN on either side compares false; -inf - logp is -inf or NaN)
    const bool acc = log(u) < (lpp - lp) + lj;          // (wave-uniform)
    const int nr = a.nrows[w];
    // a chain that has overflowed (or whose row count is not one the store can hold) records
    // nothing any more
    const bool recording = a.overflow[w] == 0 && nr >= 1 && nr <= a.cap;
    const bool new_row = recording && acc && nr < a.cap;
    const int64_t n = a.nstat[w] + 1;
    const int64_t base = (int64_t)w * a.nfree;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int f = lane + h * kWave;
        if (f >= a.nfree)
            continue;
        double x = a.theta[base + f];
        if (acc) {
            x = a.prop[base + f];
            a.theta[base + f] = x;
        }
        // Welford's update with the state after the decision
        double mean = a.mean[base + f];
        const double delta = x - mean;
        mean = mean + delta / (double)n;
        a.mean[base + f] = mean;
        a.m2[base + f] = a.m2[base + f] + delta * (x - mean);
        if (a.append)
            a.z[(a.M + w) * a.nfree + f] = x;
        if (new_row)
            a.rows[((int64_t)w * a.cap + nr) * a.nfree + f] = x;
    }
    if (lane != 0)
        return;
    if (acc)
        a.logp[w] = lpp;
    a.accepted[w] = acc ? 1 : 0;
    a.nstat[w] = n;
    if (!recording)
        return;
    const int64_t slot = (int64_t)w * a.cap;
    if (new_row) {
        a.row_logp[slot + nr] = lpp;
        a.row_gen[slot + nr] = (int32_t)a.g;
        a.counts[slot + nr] = 1;
        a.nrows[w] = nr + 1;
    } else if (acc) {
        a.overflow[w] = 1;
    } else {
        a.counts[slot + nr - 1] += 1;
    }
}

// One thread per parameter, the chains in their order.
__global__ __launch_bounds__(kWave) void k_gelman_rubin(
    double *__restrict__ rhat, const double *__restrict__ mean, const double *__restrict__ m2,
    int64_t n, int nfree, int nw)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nfree)
        return;
    if (n < 2 || nw < 2) {
        rhat[f] = NAN;
        return;
    }
    double sum_var = 0.0, sum_mean = 0.0;
    for (int w = 0; w < nw; w++) {
        sum_var += m2[(int64_t)w * nfree + f] / (double)(n - 1);
        sum_mean += mean[(int64_t)w * nfree + f];
    }
    const double W = sum_var / (double)nw;
    const double grand = sum_mean / (double)nw;
    double ss = 0.0;
    for (int w = 0; w < nw; w++) {
        const double dev = mean[(int64_t)w * nfree + f] - grand;
        ss += dev * dev;
    }
    const double b_over_n = ss / (double)(nw - 1);
    const double v = ((double)(n - 1) / (double)n) * W + b_over_n;
    rhat[f] = W == 0.0 ? NAN : sqrt(v / W);
}

__global__ __launch_bounds__(256) void k_philox_uniform(double *__restrict__ out, uint64_t seed,
                                                        int ncol, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total)
        return;
    const int64_t row = i / ncol;
    const int col = (int)(i - row * ncol);
    const pb::PhiloxWords r = pb::philox_block(seed, (uint32_t)(col >> 1), (uint32_t)row, 0u,
                                               pb::kTagInitial);
    out[i] = (col & 1) ? pb::philox_u01(r.x[2], r.x[3]) : pb::philox_u01(r.x[0], r.x[1]);
}

constexpr int64_t kGenerations = (int64_t)1 << 32;

}  // namespace

extern "C" {

int pb_demc_propose(double *prop_d, double *log_jac_d, int32_t *kind_d, const double *theta_d,
                    const double *z_d, const double *pstep_d, int64_t g, uint64_t seed, int64_t M,
                    double fgamma, double fepsilon, double p_snooker, int nfree, int nwalkers,
                    void *stream)
{
    PB_REQUIRE(nfree >= 1 && nwalkers >= 0, "pb_demc_propose: bad shape");
    PB_REQUIRE(nfree <= kMaxPar,
               "pb_demc_propose: %d free parameters: at most %d (a wavefront holds two per lane)",
               nfree, kMaxPar);
    PB_REQUIRE(M >= 3, "pb_demc_propose: a history of %lld rows: at least 3 (two distinct rows "
               "and the snooker's anchor)", (long long)M);
    PB_REQUIRE(g >= 0 && g < kGenerations,
               "pb_demc_propose: generation %lld: the counter holds 0 <= g < 2^32", (long long)g);
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(prop_d && log_jac_d && kind_d && theta_d && z_d && pstep_d,
               "pb_demc_propose: null pointer");
    const double gamma = fgamma * 2.38 / sqrt(2.0 * (double)nfree);
    k_demc_propose<<<pb::div_up(nwalkers, kWavesPerBlock), kWave * kWavesPerBlock, 0,
                     pb::as_stream(stream)>>>(prop_d, log_jac_d, kind_d, theta_d, z_d, pstep_d,
                                              (uint32_t)g, seed, M, gamma, fepsilon, p_snooker,
                                              nfree, nwalkers);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_demc_accept(double *theta_d, double *logp_d, const double *prop_d,
                   const double *logp_prop_d, const double *log_jac_d, double *rows_d,
                   double *row_logp_d, int32_t *row_gen_d, int64_t *counts_d, int32_t *nrows_d,
                   int32_t *overflow_d, double *mean_d, double *m2_d, int64_t *nstat_d,
                   double *z_d, int32_t *accepted_d, int64_t g, uint64_t seed, int64_t M,
                   int64_t Mcap, int append, int cap, int nfree, int nwalkers, void *stream)
{
    PB_REQUIRE(nfree >= 1 && nwalkers >= 0 && cap >= 1, "pb_demc_accept: bad shape");
    PB_REQUIRE(nfree <= kMaxPar,
               "pb_demc_accept: %d free parameters: at most %d (a wavefront holds two per lane)",
               nfree, kMaxPar);
    PB_REQUIRE(g >= 0 && g < kGenerations,
               "pb_demc_accept: generation %lld: the counter holds 0 <= g < 2^32", (long long)g);
    PB_REQUIRE(g <= INT32_MAX, "pb_demc_accept: generation %lld does not fit row_gen (int32)",
               (long long)g);
    PB_REQUIRE(!append || (M >= 0 && M + nwalkers <= Mcap),
               "pb_demc_accept: appending %d rows to a history of %lld: its capacity is %lld",
               nwalkers, (long long)M, (long long)Mcap);
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(theta_d && logp_d && prop_d && logp_prop_d && log_jac_d && rows_d && row_logp_d &&
                   row_gen_d && counts_d && nrows_d && overflow_d && mean_d && m2_d && nstat_d &&
                   accepted_d && (z_d || !append),
               "pb_demc_accept: null pointer");
    AcceptArgs a;
    a.theta = theta_d, a.logp = logp_d;
    a.prop = prop_d, a.logp_prop = logp_prop_d, a.log_jac = log_jac_d;
    a.rows = rows_d, a.row_logp = row_logp_d, a.row_gen = row_gen_d, a.counts = counts_d;
    a.nrows = nrows_d, a.overflow = overflow_d;
    a.mean = mean_d, a.m2 = m2_d, a.nstat = nstat_d;
    a.z = z_d, a.accepted = accepted_d;
    a.seed = seed, a.M = M, a.g = (uint32_t)g;
    a.append = append ? 1 : 0, a.cap = cap, a.nfree = nfree, a.nw = nwalkers;
    k_demc_accept<<<pb::div_up(nwalkers, kWavesPerBlock), kWave * kWavesPerBlock, 0,
                    pb::as_stream(stream)>>>(a);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_gelman_rubin(double *rhat_d, const double *mean_d, const double *m2_d, int64_t n,
                    int nfree, int nwalkers, void *stream)
{
    PB_REQUIRE(nfree >= 1 && nwalkers >= 0 && n >= 0, "pb_gelman_rubin: bad shape");
    PB_REQUIRE(rhat_d && (nwalkers == 0 || (mean_d && m2_d)), "pb_gelman_rubin: null pointer");
    k_gelman_rubin<<<pb::div_up(nfree, kWave), kWave, 0, pb::as_stream(stream)>>>(
        rhat_d, mean_d, m2_d, n, nfree, nwalkers);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_philox_uniform(double *out_d, uint64_t seed, int64_t n, int ncol, void *stream)
{
    PB_REQUIRE(n >= 0 && ncol >= 1, "pb_philox_uniform: bad shape");
    PB_REQUIRE(n < kGenerations, "pb_philox_uniform: %lld rows: the counter holds fewer than 2^32",
               (long long)n);
    if (n == 0)
        return PB_OK;
    PB_REQUIRE(out_d, "pb_philox_uniform: null pointer");
    const int64_t total = n * ncol;
    k_philox_uniform<<<pb::div_up(total, 256), 256, 0, pb::as_stream(stream)>>>(out_d, seed, ncol,
                                                                              total);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
