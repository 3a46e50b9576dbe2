// The front end of the batched retrieval loop, towards the sampler: the sampler's matrix
// theta[nw, nfree] of free parameters -> every per-walker tensor the loop takes, the log-prior and
// the bounds flag (k_retrieval_map; the reference's index maps of pyrat/retrieval.py:167-284 as
// pyrat_obj.py:258-297 applies them, with Loglike's free / fixed / shared rule,
// tools/retrieval_tools.py:45-46, 91-93), the prior transform of a nested sampler
// (k_prior_transform) and the combine of log-likelihood, log-prior and bounds flag
// (k_log_posterior).  Plain launches: no allocation, no synchronisation.
#include "pb_common.h"

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kMaxPar = PB_RETRIEVAL_MAX_PARAMS;
constexpr int kMaxDest = PB_RETRIEVAL_MAX_DESTS;
static_assert(kMaxPar == 2 * kWave, "k_retrieval_map gives every lane two parameters");

// the destination tensors of one call, by value in the kernel's arguments
struct MapDests {
    double *ptr[kMaxDest];       // [nw, ncols[d]]
    int32_t ncols[kMaxDest];
};

// the two-sided Gaussian's term of one free parameter; uniform (lo == up == 0): 0
__device__ __forceinline__ double prior_term(double p, double prior, double lo, double up)
{
    if (lo == 0.0 && up == 0.0)
        return 0.0;
    const double s = p < prior ? lo : up;
    const double z = (p - prior) / s;
    return -0.5 * (z * z);
}

// One wavefront per walker, lanes over parameters (lane and lane + 64).  The bounds test comes
// first; a walker that fails it is mapped from `value` (the block's value column of the free
// parameters) instead of its own row, so that no later kernel sees NaN or out-of-range input, and
// its log-prior is -inf.  The prior is summed in a fixed order: lane l holds term[l] + term[l + 64],
// then a butterfly -- the same bits in every run.
__global__ __launch_bounds__(kWave * kWavesPerBlock) void k_retrieval_map(
    MapDests dests, double *__restrict__ log_prior, int32_t *__restrict__ inside,
    const double *__restrict__ theta, const int32_t *__restrict__ src,
    const double *__restrict__ cons, const double *__restrict__ factor,
    const int32_t *__restrict__ dest, const int32_t *__restrict__ col,
    const double *__restrict__ value, const double *__restrict__ pmin,
    const double *__restrict__ pmax, const double *__restrict__ prior,
    const double *__restrict__ priorlow, const double *__restrict__ priorup, int nmap, int nfree,
    int ndest, int nw)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int w = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (w >= nw)                                        // (wave-uniform)
        return;
    const double *row = theta + (int64_t)w * nfree;
    bool ok = true;
    double acc = 0.0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int f = lane + h * kWave;
        if (f < nfree) {
            const double p = row[f];
            ok = ok && isfinite(p) && p >= pmin[f] && p <= pmax[f];
            acc += prior_term(p, prior[f], priorlow[f], priorup[f]);
        }
    }
    const bool in = __all(ok);
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1)
        acc += __shfl_xor(acc, d);
    if (lane == 0) {
        log_prior[w] = in ? acc : -INFINITY;
        inside[w] = in ? 1 : 0;
    }
    const double *from = in ? row : value;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int e = lane + h * kWave;
        if (e >= nmap)
            continue;
        // (an entry that points outside its destination or outside theta writes nothing)
        const int d = dest[e];
        const int s = src[e];
        if (d < 0 || d >= ndest || s >= nfree)
            continue;
        if (col[e] < 0 || col[e] >= dests.ncols[d])
            continue;
        double v = s >= 0 ? from[s] : cons[e];
        const double fac = factor[e];
        if (fac != 1.0)
            v = v * fac;
        dests.ptr[d][(int64_t)w * dests.ncols[d] + col[e]] = v;
    }
}

// u (lo + up) < lo, the side of prior an element of the unit cube falls on, decided exactly: the
// sum lo + up with its rounding error (two-sum), u times that sum with its rounding error (one
// fma), and a difference p - lo that is exact near the split.  fl(lo / (lo + up)) lies an ulp or
// two off the split, and a u between the two is computed by the other side's statement: right to
// first order, but with the rounding of the OTHER side's width, a thousand units of
// eps (|prior| + s (1 + |z|)) where lo = 1000 up.  (The build's -ffp-contract=off keeps these
// operations apart.)  u = 0: below; u = 1 and NaN: not below.
__device__ __forceinline__ bool below_split(double u, double lo, double up)
{
    const double s = lo + up;
    const double t = s - lo;
    const double es = (lo - (s - t)) + (up - t);
    const double p = u * s;
    const double ep = fma(u, s, -p);
    return (p - lo) + (ep + u * es) < 0.0;
}

// theta[w, f] from the unit cube: uniform: pmin + u (pmax - pmin); two-sided Gaussian: the inverse
// CDF of the density exp(-0.5 ((p - prior) / s)^2), s = lo below prior and up above it, whose mass
// below prior is lo / (lo + up).  Either branch hands normcdfinv the tail mass itself: above prior
// -normcdfinv(x), not normcdfinv(1 - x), which loses the tail from three sigma upward.  u = 0
// gives -inf, u = 1 +inf.  Not truncated to [pmin, pmax].
__global__ __launch_bounds__(256) void k_prior_transform(
    double *__restrict__ theta, const double *__restrict__ cube, const double *__restrict__ pmin,
    const double *__restrict__ pmax, const double *__restrict__ prior,
    const double *__restrict__ priorlow, const double *__restrict__ priorup, int nfree,
    int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total)
        return;
    const int f = (int)(i % nfree);
    const double u = cube[i];
    const double lo = priorlow[f], up = priorup[f];
    double v;
    if (lo == 0.0 && up == 0.0) {
        v = pmin[f] + u * (pmax[f] - pmin[f]);
    } else if (below_split(u, lo, up)) {
        v = prior[f] + lo * normcdfinv(0.5 * u * (lo + up) / lo);
    } else {
        v = prior[f] - up * normcdfinv(0.5 * (1.0 - u) * (1.0 + lo / up));
    }
    theta[i] = v;
}

__global__ __launch_bounds__(256) void k_log_posterior(
    double *__restrict__ out, const double *__restrict__ loglike,
    const double *__restrict__ log_prior, const int32_t *__restrict__ inside, double outside_value,
    int add_prior, int nw)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw)
        return;
    double v = outside_value;
    if (inside[w] != 0)
        v = add_prior ? loglike[w] + log_prior[w] : loglike[w];
    out[w] = v;
}

}  // namespace

extern "C" {

int pb_retrieval_map(double *const *dest_ptrs, const int32_t *dest_ncols, int ndest,
                     double *log_prior_d, int32_t *inside_d, const double *theta_d,
                     const int32_t *src_d, const double *const_d, const double *factor_d,
                     const int32_t *dest_d, const int32_t *col_d, const double *value_d,
                     const double *pmin_d, const double *pmax_d, const double *prior_d,
                     const double *priorlow_d, const double *priorup_d, int nmap, int nfree,
                     int nwalkers, void *stream)
{
    PB_REQUIRE(nmap >= 1 && nfree >= 1 && nwalkers >= 0 && ndest >= 0,
               "pb_retrieval_map: bad shape");
    PB_REQUIRE(nmap <= kMaxPar && nfree <= kMaxPar,
               "pb_retrieval_map: %d mapped and %d free parameters: at most %d of either (a "
               "wavefront holds two per lane)", nmap, nfree, kMaxPar);
    PB_REQUIRE(ndest <= kMaxDest, "pb_retrieval_map: %d destinations: at most %d", ndest,
               kMaxDest);
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(log_prior_d && inside_d && theta_d && src_d && const_d && factor_d && dest_d &&
                   col_d && value_d && pmin_d && pmax_d && prior_d && priorlow_d && priorup_d,
               "pb_retrieval_map: null pointer");
    PB_REQUIRE(ndest == 0 || (dest_ptrs && dest_ncols),
               "pb_retrieval_map: null pointer (destinations)");
    MapDests dests = {};
    for (int d = 0; d < ndest; d++) {
        PB_REQUIRE(dest_ptrs[d] && dest_ncols[d] >= 1,
                   "pb_retrieval_map: destination %d: null pointer or no column", d);
        dests.ptr[d] = dest_ptrs[d];
        dests.ncols[d] = dest_ncols[d];
    }
    k_retrieval_map<<<pb::div_up(nwalkers, kWavesPerBlock), kWave * kWavesPerBlock, 0,
                      pb::as_stream(stream)>>>(
        dests, log_prior_d, inside_d, theta_d, src_d, const_d, factor_d, dest_d, col_d, value_d,
        pmin_d, pmax_d, prior_d, priorlow_d, priorup_d, nmap, nfree, ndest, nwalkers);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_prior_transform(double *theta_d, const double *cube_d, const double *pmin_d,
                       const double *pmax_d, const double *prior_d, const double *priorlow_d,
                       const double *priorup_d, int nfree, int nwalkers, void *stream)
{
    PB_REQUIRE(nfree >= 1 && nwalkers >= 0, "pb_prior_transform: bad shape");
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(theta_d && cube_d && pmin_d && pmax_d && prior_d && priorlow_d && priorup_d,
               "pb_prior_transform: null pointer");
    const int64_t total = (int64_t)nwalkers * nfree;
    k_prior_transform<<<pb::div_up(total, 256), 256, 0, pb::as_stream(stream)>>>(
        theta_d, cube_d, pmin_d, pmax_d, prior_d, priorlow_d, priorup_d, nfree, total);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_log_posterior(double *out_d, const double *loglike_d, const double *log_prior_d,
                     const int32_t *inside_d, double outside_value, int add_prior, int nwalkers,
                     void *stream)
{
    PB_REQUIRE(nwalkers >= 0, "pb_log_posterior: bad shape");
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(out_d && loglike_d && inside_d && (log_prior_d || !add_prior),
               "pb_log_posterior: null pointer");
    k_log_posterior<<<pb::div_up(nwalkers, 256), 256, 0, pb::as_stream(stream)>>>(
        out_d, loglike_d, log_prior_d, inside_d, outside_value, add_prior, nwalkers);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
