// Nested sampling for the batched retrieval loop (Skilling 2006): per iteration the K lowest of
// nlive live points die at once and K walkers replace them, so that one walk step is one batch:
// k_nested_rank + k_nested_weights -> nsteps x (k_nested_propose -> the caller's prior transform
// and log-likelihood -> k_nested_accept); k_nested_finish and k_nested_resample make the result.
// The NumPy statements of pyratbay_amd/nested.py (select_host, start_host, propose_host,
// accept_host, finish_host, resample_host) are the specification; pb_philox.h gives both sides
// the same random words.
//
// The walk's kernels: one wavefront per slot, the free parameters two per lane (lane and
// lane + 64, as k_demc_propose).  Ranking counts over the live log-likelihoods held in LDS: the
// order depends on the values and indices alone.  ln X, ln Z, Lstar and the stopping quantity
// live in four doubles on the device; every sum is taken in a fixed order.  Plain launches: no
// allocation, no synchronisation.
#include "pb_common.h"
#include "pb_philox.h"

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kMaxPar = PB_RETRIEVAL_MAX_PARAMS;
constexpr int kMaxLive = PB_NESTED_MAX_LIVE;
constexpr int kBlock = 256;
static_assert(kMaxPar == 2 * kWave, "the walk's kernels give every lane two parameters");
// the slots of the state
constexpr int kLnX = 0, kLnZ = 1, kLstar = 2, kRemain = 3;

// NumPy's logaddexp
__device__ __forceinline__ double log_add_exp(double x, double y)
{
    if (x == y)
        return x + 0.693147180559945309417232121458176568;
    const double d = x - y;
    if (d > 0.0)
        return x + log1p(exp(-d));
    if (d <= 0.0)
        return y + log1p(exp(d));
    return d;                                           // NaN
}

// ---- select -----------------------------------------------------------------------------------
// One thread per live point: its rank is the number of points below it -- a NaN below everything,
// equal values (and NaNs among themselves) by index.  The K lowest go to the dead store.
__global__ __launch_bounds__(kBlock) void k_nested_rank(
    int32_t *__restrict__ dead_idx, int32_t *__restrict__ surv_idx, double *__restrict__ dead_u,
    double *__restrict__ dead_logl, const double *__restrict__ live_u,
    const double *__restrict__ live_logl, int64_t dead_base, int K, int nlive, int nfree)
{
    __shared__ double key[kMaxLive];
    for (int j = threadIdx.x; j < nlive; j += kBlock)
        key[j] = live_logl[j];
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nlive)
        return;
    const double v = key[i];
    const bool vnan = v != v;
    int rank = 0;
    for (int j = 0; j < nlive; j++) {
        const double w = key[j];
        const bool wnan = w != w;
        const bool below = vnan ? (wnan && j < i) : (wnan || w < v || (w == v && j < i));
        rank += below ? 1 : 0;
    }
    if (rank >= K) {
        surv_idx[rank - K] = i;
        return;
    }
    dead_idx[rank] = i;
    dead_logl[dead_base + rank] = v;
    const double *src = live_u + (int64_t)i * nfree;
    double *dst = dead_u + (dead_base + rank) * nfree;
    for (int f = 0; f < nfree; f++)
        dst[f] = src[f];
}

// One block: the shells ln(-expm1(-1 / n)) side by side, then one thread walks the K deaths in
// their order.
__global__ __launch_bounds__(kBlock) void k_nested_weights(
    double *__restrict__ dead_logw, double *__restrict__ state,
    const double *__restrict__ dead_logl, const double *__restrict__ live_logl,
    const int32_t *__restrict__ surv_idx, int64_t dead_base, int K, int nlive)
{
    __shared__ double logl[kMaxLive], shell[kMaxLive];
    for (int j = threadIdx.x; j < K; j += kBlock) {
        logl[j] = dead_logl[dead_base + j];
        shell[j] = log(-expm1(-(1.0 / (double)(nlive - j))));
    }
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    double ln_x = state[kLnX], ln_z = state[kLnZ];
    for (int j = 0; j < K; j++) {
        const double l = logl[j];
        const double lw = (l != l) ? -HUGE_VAL : (l + ln_x) + shell[j];
        dead_logw[dead_base + j] = lw;
        ln_x = ln_x - 1.0 / (double)(nlive - j);
        ln_z = log_add_exp(ln_z, lw);
    }
    const int top = surv_idx[nlive - K - 1];
    const double ltop = (top >= 0 && top < nlive) ? live_logl[top] : NAN;
    state[kLnX] = ln_x;
    state[kLnZ] = ln_z;
    state[kLstar] = logl[K - 1];
    state[kRemain] = log_add_exp(ln_z, ltop + ln_x) - ln_z;
}

// ---- the walk ---------------------------------------------------------------------------------
struct ProposeArgs {
    double *point;                              // [K, nfree]
    int32_t *inside, *a, *b;                    // [K]
    double *gamma;                              // [K]
    double *cur, *cur_logl;                     // [K, nfree], [K]
    int32_t *acc_it;                            // [K]
    const double *live_u, *live_logl;           // [nlive, nfree], [nlive]
    const int32_t *surv_idx;                    // [nsurv]
    uint64_t seed;
    uint32_t it, q;
    double gamma_de, p_unit;
    int start, nsurv, nlive, nfree, K;
};

// a survivor's live index, kept inside the live set whatever the array holds
__device__ __forceinline__ int survivor(const ProposeArgs &p, int64_t r)
{
    const int i = p.surv_idx[r];
    return i < 0 ? 0 : (i >= p.nlive ? p.nlive - 1 : i);
}

__global__ __launch_bounds__(kWave * kWavesPerBlock) void k_nested_propose(ProposeArgs p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int k = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (k >= p.K)                                       // (wave-uniform)
        return;
    double ua, ub, um;
    double c[2] = {0.5, 0.5};
    const int64_t base = (int64_t)k * p.nfree;
    if (p.start) {
        pb::philox_block_uniforms(p.seed, 0u, (uint32_t)k, p.it, pb::kTagNestedStart, ua, ub);
        const int pick = survivor(p, pb::philox_index(ua, p.nsurv));
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int f = lane + h * kWave;
            if (f < p.nfree) {
                c[h] = p.live_u[(int64_t)pick * p.nfree + f];
                p.cur[base + f] = c[h];
            }
        }
        if (lane == 0) {
            p.cur_logl[k] = p.live_logl[pick];
            p.acc_it[k] = 0;
        }
    } else {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int f = lane + h * kWave;
            if (f < p.nfree)
                c[h] = p.cur[base + f];
        }
    }
    pb::philox_block_uniforms(p.seed, 0u, (uint32_t)k, p.q, pb::kTagNestedStep, ua, ub);
    const int64_t a = pb::philox_index(ua, p.nsurv);
    int64_t b = pb::philox_index(ub, p.nsurv - 1);
    b += (b >= a) ? 1 : 0;
    pb::philox_block_uniforms(p.seed, 1u, (uint32_t)k, p.q, pb::kTagNestedStep, um, ub);
    const double gamma = um < p.p_unit ? 1.0 : p.gamma_de;
    const double *ra = p.live_u + (int64_t)survivor(p, a) * p.nfree;
    const double *rb = p.live_u + (int64_t)survivor(p, b) * p.nfree;
    double prop[2] = {0.5, 0.5};
    bool ok = true;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int f = lane + h * kWave;
        if (f < p.nfree) {
            prop[h] = c[h] + gamma * (ra[f] - rb[f]);
            ok = ok && prop[h] > 0.0 && prop[h] < 1.0;
        }
    }
    const bool inside = __all(ok);                      // (wave-uniform)
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int f = lane + h * kWave;
        if (f < p.nfree)
            p.point[base + f] = inside ? prop[h] : c[h];
    }
    if (lane == 0) {
        p.inside[k] = inside ? 1 : 0;
        p.a[k] = (int32_t)a;
        p.b[k] = (int32_t)b;
        p.gamma[k] = gamma;
    }
}

struct WalkAcceptArgs {
    double *cur, *cur_logl;                     // [K, nfree], [K]: in place
    const double *point, *logl_prop;
    const int32_t *inside;
    const double *state;
    int64_t *naccept;                           // [K]
    int32_t *acc_it;                            // [K]
    int64_t *stuck;                             // [K]
    int32_t *accepted;                          // [K]
    double *live_u, *live_logl;                 // written with last
    const int32_t *dead_idx;                    // [K]
    int last, nlive, nfree, K;
};

__global__ __launch_bounds__(kWave * kWavesPerBlock) void k_nested_accept(WalkAcceptArgs a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int k = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (k >= a.K)                                       // (wave-uniform)
        return;
    const double lstar = a.state[kLstar], lp = a.logl_prop[k];
    // (a NaN on either side compares false)
    const bool acc = a.inside[k] != 0 && lp > lstar;    // (wave-uniform)
    const int home = a.last ? a.dead_idx[k] : -1;
    const bool write_back = home >= 0 && home < a.nlive;
    const int64_t base = (int64_t)k * a.nfree;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int f = lane + h * kWave;
        if (f >= a.nfree)
            continue;
        double x = a.cur[base + f];
        if (acc) {
            x = a.point[base + f];
            a.cur[base + f] = x;
        }
        if (write_back)
            a.live_u[(int64_t)home * a.nfree + f] = x;
    }
    if (lane != 0)
        return;
    double cl = a.cur_logl[k];
    int n_it = a.acc_it[k];
    if (acc) {
        cl = lp;
        n_it += 1;
        a.cur_logl[k] = cl;
        a.acc_it[k] = n_it;
        a.naccept[k] += 1;
    }
    a.accepted[k] = acc ? 1 : 0;
    if (a.last) {
        if (write_back)
            a.live_logl[home] = cl;
        if (n_it == 0)
            a.stuck[k] += 1;
    }
}

// ---- finish -----------------------------------------------------------------------------------
// One block.  The weights of the dead and the live points side by side, their maximum, then the
// sums in 256 chunks of consecutive rows: every thread sums its chunk in index order, one thread
// sums the chunks in chunk order, and every thread walks its chunk again from the sum of the
// chunks before it (nested._chunked_cumsum).
__device__ __forceinline__ double weight_of(double lw, double m)
{
    return lw == -HUGE_VAL ? 0.0 : exp(lw - m);
}

__global__ __launch_bounds__(kBlock) void k_nested_finish(
    double *__restrict__ out, double *__restrict__ logw, double *__restrict__ logl,
    double *__restrict__ cdf, const double *__restrict__ dead_logl,
    const double *__restrict__ dead_logw, const double *__restrict__ live_logl,
    const double *__restrict__ state, int64_t ndead, int nlive)
{
    __shared__ double part[kBlock], hpart[kBlock], before[kBlock];
    __shared__ double total[2];
    const int t = threadIdx.x;
    const int64_t n = ndead + nlive;
    const double ln_x = state[kLnX], ln_n = log((double)nlive);
    double m = -HUGE_VAL;
    for (int64_t i = t; i < n; i += kBlock) {
        double l, lw;
        if (i < ndead) {
            l = dead_logl[i];
            lw = dead_logw[i];
        } else {
            l = live_logl[i - ndead];
            lw = (l != l) ? -HUGE_VAL : (l + ln_x) - ln_n;
        }
        logl[i] = l;
        logw[i] = lw;
        m = fmax(m, lw);
    }
    part[t] = m;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (t < off)
            part[t] = fmax(part[t], part[t + off]);
        __syncthreads();
    }
    m = part[0];
    __syncthreads();
    const int64_t per = (n + kBlock - 1) / kBlock > 0 ? (n + kBlock - 1) / kBlock : 1;
    const int64_t lo = t * per < n ? t * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    double s = 0.0, hs = 0.0;
    for (int64_t i = lo; i < hi; i++) {
        const double e = weight_of(logw[i], m);
        s = s + e;
        hs = hs + (e > 0.0 ? e * logl[i] : 0.0);
    }
    part[t] = s;
    hpart[t] = hs;
    __syncthreads();
    if (t == 0) {
        double run = 0.0, hrun = 0.0;
        for (int c = 0; c < kBlock; c++) {
            before[c] = run;
            run = run + part[c];
            hrun = hrun + hpart[c];
        }
        total[0] = run;
        total[1] = hrun;
    }
    __syncthreads();
    const double S = total[0];
    double run = before[t];
    for (int64_t i = lo; i < hi; i++) {
        run = run + weight_of(logw[i], m);
        cdf[i] = run / S;
    }
    if (t == 0) {
        const double ln_z = m + log(S);
        const double info = total[1] / S - ln_z;
        out[0] = ln_z;
        out[1] = sqrt(fmax(info, 0.0) / (double)nlive);
        out[2] = info;
    }
}

// One thread per sample: the first row whose cdf exceeds the uniform, by bisection.
__global__ __launch_bounds__(kBlock) void k_nested_resample(
    unsigned long long *__restrict__ counts, const double *__restrict__ cdf, int64_t n,
    int64_t nsamples, uint64_t seed)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= nsamples)
        return;
    double ua, ub;
    pb::philox_block_uniforms(seed, 0u, (uint32_t)(s >> 1), 0u, pb::kTagNestedResample, ua, ub);
    const double u = (s & 1) ? ub : ua;
    int64_t lo = 0, hi = n;                             // the answer lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > u)
            hi = mid;
        else
            lo = mid + 1;
    }
    atomicAdd(counts + (lo < n - 1 ? lo : n - 1), 1ull);
}

constexpr int64_t kCounter = (int64_t)1 << 32;

}  // namespace

#define PB_NESTED_SHAPE(name, K, nlive, nfree)                                                   \
    do {                                                                                         \
        PB_REQUIRE((nfree) >= 1 && (nlive) >= 0, name ": bad shape");                            \
        PB_REQUIRE((nfree) <= kMaxPar,                                                           \
                   name ": %d free parameters: at most %d (a wavefront holds two per lane)",     \
                   (nfree), kMaxPar);                                                            \
        PB_REQUIRE((nlive) <= kMaxLive, name ": %d live points: at most %d", (nlive), kMaxLive); \
        PB_REQUIRE((K) >= 1 && (K) <= (nlive)-2,                                                 \
                   name ": a batch of %d with %d live points: 1 <= batch <= nlive - 2", (K),     \
                   (nlive));                                                                     \
    } while (0)

extern "C" {

int pb_nested_select(int32_t *dead_idx_d, int32_t *surv_idx_d, double *dead_u_d,
                     double *dead_logl_d, double *dead_logw_d, double *state_d,
                     const double *live_u_d, const double *live_logl_d, int64_t dead_base,
                     int64_t dead_cap, int K, int nlive, int nfree, void *stream)
{
    PB_NESTED_SHAPE("pb_nested_select", K, nlive, nfree);
    PB_REQUIRE(dead_base >= 0 && dead_base + K <= dead_cap,
               "pb_nested_select: %d rows behind %lld dead points: the store holds %lld", K,
               (long long)dead_base, (long long)dead_cap);
    PB_REQUIRE(dead_idx_d && surv_idx_d && dead_u_d && dead_logl_d && dead_logw_d && state_d &&
                   live_u_d && live_logl_d,
               "pb_nested_select: null pointer");
    hipStream_t s = pb::as_stream(stream);
    k_nested_rank<<<pb::div_up(nlive, kBlock), kBlock, 0, s>>>(
        dead_idx_d, surv_idx_d, dead_u_d, dead_logl_d, live_u_d, live_logl_d, dead_base, K, nlive,
        nfree);
    PB_LAUNCH_CHECK();
    k_nested_weights<<<1, kBlock, 0, s>>>(dead_logw_d, state_d, dead_logl_d, live_logl_d,
                                          surv_idx_d, dead_base, K, nlive);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_nested_propose(double *point_d, int32_t *inside_d, int32_t *a_d, int32_t *b_d,
                      double *gamma_d, double *cur_d, double *cur_logl_d, int32_t *acc_it_d,
                      const double *live_u_d, const double *live_logl_d,
                      const int32_t *surv_idx_d, int64_t it, int64_t q, uint64_t seed,
                      double fgamma, double p_unit, int start, int nlive, int nfree, int K,
                      void *stream)
{
    if (K == 0)
        return PB_OK;
    PB_NESTED_SHAPE("pb_nested_propose", K, nlive, nfree);
    PB_REQUIRE(it >= 0 && it < kCounter,
               "pb_nested_propose: iteration %lld: the counter holds 0 <= it < 2^32",
               (long long)it);
    PB_REQUIRE(q >= 0 && q < kCounter,
               "pb_nested_propose: step %lld: the counter holds 0 <= q < 2^32", (long long)q);
    PB_REQUIRE(point_d && inside_d && a_d && b_d && gamma_d && cur_d && cur_logl_d && acc_it_d &&
                   live_u_d && live_logl_d && surv_idx_d,
               "pb_nested_propose: null pointer");
    ProposeArgs p;
    p.point = point_d, p.inside = inside_d, p.a = a_d, p.b = b_d, p.gamma = gamma_d;
    p.cur = cur_d, p.cur_logl = cur_logl_d, p.acc_it = acc_it_d;
    p.live_u = live_u_d, p.live_logl = live_logl_d, p.surv_idx = surv_idx_d;
    p.seed = seed, p.it = (uint32_t)it, p.q = (uint32_t)q;
    p.gamma_de = fgamma * 2.38 / sqrt(2.0 * (double)nfree), p.p_unit = p_unit;
    p.start = start ? 1 : 0, p.nsurv = nlive - K, p.nlive = nlive, p.nfree = nfree, p.K = K;
    k_nested_propose<<<pb::div_up(K, kWavesPerBlock), kWave * kWavesPerBlock, 0,
                       pb::as_stream(stream)>>>(p);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_nested_accept(double *cur_d, double *cur_logl_d, const double *point_d,
                     const double *logl_prop_d, const int32_t *inside_d, const double *state_d,
                     int64_t *naccept_d, int32_t *acc_it_d, int64_t *stuck_d, int32_t *accepted_d,
                     double *live_u_d, double *live_logl_d, const int32_t *dead_idx_d, int last,
                     int nlive, int nfree, int K, void *stream)
{
    if (K == 0)
        return PB_OK;
    PB_NESTED_SHAPE("pb_nested_accept", K, nlive, nfree);
    PB_REQUIRE(cur_d && cur_logl_d && point_d && logl_prop_d && inside_d && state_d &&
                   naccept_d && acc_it_d && stuck_d && accepted_d &&
                   (!last || (live_u_d && live_logl_d && dead_idx_d)),
               "pb_nested_accept: null pointer");
    WalkAcceptArgs a;
    a.cur = cur_d, a.cur_logl = cur_logl_d, a.point = point_d, a.logl_prop = logl_prop_d;
    a.inside = inside_d, a.state = state_d, a.naccept = naccept_d, a.acc_it = acc_it_d;
    a.stuck = stuck_d, a.accepted = accepted_d, a.live_u = live_u_d, a.live_logl = live_logl_d;
    a.dead_idx = dead_idx_d;
    a.last = last ? 1 : 0, a.nlive = nlive, a.nfree = nfree, a.K = K;
    k_nested_accept<<<pb::div_up(K, kWavesPerBlock), kWave * kWavesPerBlock, 0,
                      pb::as_stream(stream)>>>(a);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_nested_finish(double *out_d, double *logw_d, double *logl_d, double *cdf_d,
                     const double *dead_logl_d, const double *dead_logw_d,
                     const double *live_logl_d, const double *state_d, int64_t ndead, int nlive,
                     void *stream)
{
    PB_REQUIRE(ndead >= 0 && nlive >= 1, "pb_nested_finish: bad shape");
    PB_REQUIRE(nlive <= kMaxLive, "pb_nested_finish: %d live points: at most %d", nlive,
               kMaxLive);
    PB_REQUIRE(out_d && logw_d && logl_d && cdf_d && live_logl_d && state_d &&
                   (ndead == 0 || (dead_logl_d && dead_logw_d)),
               "pb_nested_finish: null pointer");
    k_nested_finish<<<1, kBlock, 0, pb::as_stream(stream)>>>(
        out_d, logw_d, logl_d, cdf_d, dead_logl_d, dead_logw_d, live_logl_d, state_d, ndead,
        nlive);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_nested_resample(int64_t *counts_d, const double *cdf_d, int64_t n, int64_t nsamples,
                       uint64_t seed, void *stream)
{
    PB_REQUIRE(n >= 1 && nsamples >= 0, "pb_nested_resample: bad shape");
    PB_REQUIRE(nsamples <= kCounter, "pb_nested_resample: %lld samples: at most 2^32",
               (long long)nsamples);
    PB_REQUIRE(counts_d && cdf_d, "pb_nested_resample: null pointer");
    hipStream_t s = pb::as_stream(stream);
    PB_HIP(hipMemsetAsync(counts_d, 0, (size_t)n * sizeof(int64_t), s));
    if (nsamples == 0)
        return PB_OK;
    k_nested_resample<<<pb::div_up(nsamples, kBlock), kBlock, 0, s>>>(
        (unsigned long long *)counts_d, cdf_d, n, nsamples, seed);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
