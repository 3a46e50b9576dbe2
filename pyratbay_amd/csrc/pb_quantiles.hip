// Weighted column quantiles: the reduction of a posterior's models to its median and credible
// bounds (posterior_post_processing, pyratbay/tools/retrieval_tools.py:384-503: np.percentile of
// models[uinv] per wavenumber / band / layer), without the expansion models[uinv] and without a
// sort.
//
// Every column values[c][0..n) is a sample whose element i occurs counts[i] times.  The element of
// rank r of the sorted virtual expansion is found by a weighted radix select on the
// order-preserving 64-bit key of the double (sign bit flipped for positives, every bit for
// negatives): from the highest bit in which the keys of the column differ downwards, 8 bits per
// pass, a histogram of COUNTS over the elements that share the prefix found so far; the bin whose
// running sum passes the rank is the next digit.  The histograms are 64-bit integer LDS atomics --
// exact, so the result does not depend on the order of arrival -- and ties need no care: equal
// keys share every bin.  All target ranks of a call (rank_lo and rank_hi of up to kTargets / 2
// quantiles at a time) are resolved in the same passes: targets with the same prefix share a
// histogram (the first of them, its leader, owns it), an element adds to the one histogram whose
// prefix it matches.  Passes above the highest differing bit are skipped (the keys' minimum and
// maximum come out of the first read), which also spreads the first histogram: the spectra of a
// posterior agree in their leading bytes, and a pass over those would put every add on one bin.
//
// One workgroup of 512 threads per column, a grid-stride loop over the columns.  Two regimes of
// the same code: n <= kResident stages the column's keys in LDS (one read of values from HBM);
// above, every pass re-reads the column (L2).  counts are read from global memory in every pass
// (one vector shared by all columns).
#include "pb_common.h"

#include <cmath>

namespace {

using u64 = unsigned long long;
using i64 = long long;

constexpr int kThreads = 512;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kBins = 256;
constexpr int kTargets = 12;                  // target ranks resolved together (6 quantiles)
constexpr int kUnroll = 8;                    // loads in flight per thread in a pass
// LDS in 8-byte words: the histograms, then {prefix, next prefix, rank, next rank}[kTargets],
// leader[kTargets] (int, 8 words), {min key, max key, sum of counts} (8 words), then the keys
constexpr int kHistWords = kTargets * kBins;
constexpr int kStateWords = 4 * kTargets + 16;
constexpr int kFixedWords = kHistWords + kStateWords;
constexpr int kLdsBytes = 160 * 1024;
// the largest column the on-chip path takes: 16384 keys (128 KiB) beside 24.6 KiB of histograms
// and state, inside the 160 KiB a workgroup may use
constexpr int kResident = 16384;
static_assert((kFixedWords + kResident) * 8 <= kLdsBytes, "LDS budget");
static_assert(kBins == 4 * kWave, "a lane scans 4 bins");

__device__ __forceinline__ u64 to_key(double v)
{
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double from_key(u64 k)
{
    const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((i64)b);
}

// NumPy's _lerp (numpy/lib/_function_base_impl.py), every operation rounded on its own
__device__ __forceinline__ double lerp_numpy(double a, double b, double t)
{
    const double d = __dsub_rn(b, a);
    if (t >= 0.5)
        return __dsub_rn(b, __dmul_rn(d, __dsub_rn(1.0, t)));
    return __dadd_rn(a, __dmul_rn(d, t));
}

template <bool kRes>
__global__ __launch_bounds__(kThreads, 4) void k_weighted_quantiles(
    double *__restrict__ out, const double *__restrict__ values, int64_t ld,
    const int64_t *__restrict__ counts, int n, int ncol, const int64_t *__restrict__ rank_lo,
    const int64_t *__restrict__ rank_hi, const double *__restrict__ gamma, int nq)
{
    extern __shared__ u64 s_mem[];
    u64 *s_hist = s_mem;
    u64 *s_prefix = s_mem + kHistWords;
    u64 *s_nprefix = s_prefix + kTargets;
    i64 *s_rank = reinterpret_cast<i64 *>(s_nprefix + kTargets);
    i64 *s_nrank = s_rank + kTargets;
    int *s_leader = reinterpret_cast<int *>(s_nrank + kTargets);
    u64 *s_red = s_mem + kHistWords + 4 * kTargets + 8;
    u64 *s_keys = s_mem + kFixedWords;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid / kWave;

    for (int c = blockIdx.x; c < ncol; c += gridDim.x) {
        const double *col = values + (int64_t)c * ld;
        __syncthreads();                       // (the last column's readers of s_red are done)
        if (tid < 3)
            s_red[tid] = tid == 0 ? ~0ull : 0ull;
        __syncthreads();
        // the one read of the column: its keys (staged when resident), the range of the keys of
        // the rows that exist and the length N of the expansion
        u64 kmin = ~0ull, kmax = 0ull, total = 0ull;
        for (int i0 = tid; i0 < n; i0 += kUnroll * kThreads) {
            double v[kUnroll];
            i64 w[kUnroll];
#pragma unroll
            for (int j = 0; j < kUnroll; j++) {            // (a sweep's loads in flight together)
                const int i = i0 + j * kThreads;
                v[j] = i < n ? col[i] : 0.0;
                w[j] = i < n ? counts[i] : 0;
            }
#pragma unroll
            for (int j = 0; j < kUnroll; j++) {
                const int i = i0 + j * kThreads;
                if (i >= n)
                    continue;
                const u64 k = to_key(v[j]);
                if (kRes)
                    s_keys[i] = k;
                if (w[j] > 0) {
                    kmin = k < kmin ? k : kmin;
                    kmax = k > kmax ? k : kmax;
                    total += (u64)w[j];
                }
            }
        }
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const u64 lo = __shfl_xor(kmin, off, kWave), hi = __shfl_xor(kmax, off, kWave);
            kmin = lo < kmin ? lo : kmin;
            kmax = hi > kmax ? hi : kmax;
            total += __shfl_xor(total, off, kWave);
        }
        if (lane == 0) {
            atomicMin(&s_red[0], kmin);
            atomicMax(&s_red[1], kmax);
            atomicAdd(&s_red[2], total);
        }
        __syncthreads();
        kmin = s_red[0];
        kmax = s_red[1];
        total = s_red[2];
        if (total == 0) {                      // no row exists: NaN (the caller's error)
            for (int q = tid; q < nq; q += kThreads)
                out[(int64_t)q * ncol + c] = NAN;
            continue;
        }
        // the keys agree above bit `bits`
        const int bits = kmin == kmax ? 0 : 64 - __clzll((i64)(kmin ^ kmax));

        for (int q0 = 0; q0 < nq; q0 += kTargets / 2) {
            const int nqb = nq - q0 < kTargets / 2 ? nq - q0 : kTargets / 2;
            const int T = 2 * nqb;             // target 2 j: rank_lo[q0 + j], 2 j + 1: rank_hi
            if (tid < T) {
                i64 r = (tid & 1) ? rank_hi[q0 + (tid >> 1)] : rank_lo[q0 + (tid >> 1)];
                if (r < 0 || (u64)r >= total)
                    r = -1;                    // no such element: NaN
                s_nprefix[tid] = bits == 64 ? 0ull : kmin >> bits;
                s_nrank[tid] = r;
            }
            __syncthreads();
            int hi = bits;
            while (true) {
                // the targets' state after the last pass; the leader of a target = the first
                // target with its prefix (-1: a target that has no element)
                if (tid < T) {
                    // (every target's state read first: one wait, not a chain of LDS round trips;
                    // slots from T on hold stale words that no comparison uses)
                    u64 pp[kTargets];
                    i64 rr[kTargets];
#pragma unroll
                    for (int u = 0; u < kTargets; u++) {
                        pp[u] = s_nprefix[u];
                        rr[u] = s_nrank[u];
                    }
                    const u64 p = s_nprefix[tid];
                    const i64 r = s_nrank[tid];
                    int lead = -1;
                    if (r >= 0) {
                        lead = tid;
#pragma unroll
                        for (int u = kTargets - 1; u >= 0; u--)
                            if (u < tid && rr[u] >= 0 && pp[u] == p)
                                lead = u;
                    }
                    s_prefix[tid] = p;
                    s_rank[tid] = r;
                    s_leader[tid] = lead;
                }
                if (hi == 0)
                    break;
                const int lo = hi > 8 ? hi - 8 : 0;
                const int width = hi - lo;
                for (int i = tid; i < T * kBins; i += kThreads)
                    s_hist[i] = 0ull;
                __syncthreads();
                // the histograms of counts: an element adds to the leader whose prefix it has
                {
                    u64 gp[kTargets];
                    unsigned leaders = 0;
#pragma unroll
                    for (int u = 0; u < kTargets; u++) {
                        gp[u] = u < T ? s_prefix[u] : 0ull;
                        if (u < T && s_leader[u] == u)
                            leaders |= 1u << u;
                    }
                    const u64 dmask = (1ull << width) - 1;
                    for (int i0 = tid; i0 < n; i0 += kUnroll * kThreads) {
                        u64 k[kUnroll];
                        i64 w[kUnroll];
#pragma unroll
                        for (int j = 0; j < kUnroll; j++) {
                            const int i = i0 + j * kThreads;
                            w[j] = i < n ? counts[i] : 0;
                            k[j] = i < n ? (kRes ? s_keys[i] : to_key(col[i])) : 0ull;
                        }
#pragma unroll
                        for (int j = 0; j < kUnroll; j++) {
                            if (w[j] <= 0)
                                continue;
                            const u64 p = hi == 64 ? 0ull : k[j] >> hi;
                            int slot = -1;
#pragma unroll
                            for (int u = 0; u < kTargets; u++)
                                if (((leaders >> u) & 1u) && gp[u] == p)
                                    slot = u;
                            if (slot >= 0)
                                atomicAdd(&s_hist[slot * kBins + (int)((k[j] >> lo) & dmask)],
                                          (u64)w[j]);
                        }
                    }
                }
                __syncthreads();
                // the next digit of every target: a wavefront per histogram, 4 bins per lane, the
                // running sum over the lanes by shuffles; the bin that holds the rank
                for (int u = wave; u < T; u += kWaves) {
                    if (s_leader[u] != u)
                        continue;
                    u64 h[4];
                    u64 sum = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        h[b] = s_hist[u * kBins + 4 * lane + b];
                        sum += h[b];
                    }
                    u64 incl = sum;
                    for (int off = 1; off < kWave; off <<= 1) {
                        const u64 up = __shfl_up(incl, off, kWave);
                        if (lane >= off)
                            incl += up;
                    }
                    const u64 before = incl - sum;
                    int lead[kTargets];
                    u64 rk[kTargets], pf[kTargets];
#pragma unroll
                    for (int v = 0; v < kTargets; v++) {           // (as above: one wait)
                        lead[v] = s_leader[v];
                        rk[v] = (u64)s_rank[v];
                        pf[v] = s_prefix[v];
                    }
#pragma unroll
                    for (int v = 0; v < kTargets; v++) {
                        if (v >= T || lead[v] != u)
                            continue;
                        const u64 r = rk[v];
                        u64 e = before, rest = 0;
                        int digit = -1;
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            if (h[b] > 0 && r >= e && r - e < h[b]) {
                                digit = 4 * lane + b;
                                rest = r - e;
                            }
                            e += h[b];
                        }
                        const int found = __any(digit >= 0);
                        if (digit >= 0) {
                            s_nprefix[v] = (hi == 64 ? 0ull : pf[v] << width) | (u64)digit;
                            s_nrank[v] = (i64)rest;
                        } else if (!found && lane == 0) {
                            s_nrank[v] = -1;
                        }
                    }
                }
                __syncthreads();
                hi = lo;
            }
            __syncthreads();
            if (tid < nqb) {
                double r = NAN;
                if (s_rank[2 * tid] >= 0 && s_rank[2 * tid + 1] >= 0)
                    r = lerp_numpy(from_key(s_prefix[2 * tid]), from_key(s_prefix[2 * tid + 1]),
                                   gamma[q0 + tid]);
                out[(int64_t)(q0 + tid) * ncol + c] = r;
            }
        }
    }
}

}  // namespace

extern "C" {

int pb_weighted_quantiles_resident_rows(void)
{
    return kResident;
}

int64_t pb_weighted_quantiles_work_doubles(int n, int ncol, int nq)
{
    (void)n;
    (void)ncol;
    (void)nq;
    return 0;                                  // (the selection keeps its state in LDS)
}

int pb_weighted_quantiles(double *out_d, const double *values_d, int64_t ld,
                          const int64_t *counts_d, int n, int ncol, const int64_t *rank_lo_d,
                          const int64_t *rank_hi_d, const double *gamma_d, int nq, double *work_d,
                          void *stream)
{
    PB_REQUIRE(n >= 1 && nq >= 1 && ncol >= 0 && ld >= n,
               "pb_weighted_quantiles: n = %d rows (>= 1), nq = %d quantiles (>= 1), ncol = %d "
               "columns (>= 0), ld = %lld (>= n)", n, nq, ncol, (long long)ld);
    if (ncol == 0)
        return PB_OK;
    PB_REQUIRE(out_d && values_d && counts_d && rank_lo_d && rank_hi_d && gamma_d,
               "pb_weighted_quantiles: null pointer");
    PB_REQUIRE(work_d || pb_weighted_quantiles_work_doubles(n, ncol, nq) == 0,
               "pb_weighted_quantiles: null work (pb_weighted_quantiles_work_doubles doubles of "
               "device scratch)");
    const bool resident = n <= kResident;
    const size_t lds = ((size_t)kFixedWords + (resident ? n : 0)) * sizeof(u64);
    auto kern = resident ? k_weighted_quantiles<true> : k_weighted_quantiles<false>;
    if (lds > 64 * 1024)
        PB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int device = 0, cus = 0;
    PB_HIP(hipGetDevice(&device));
    PB_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    // workgroups of 8 wavefronts: 2 per CU at the kernel's registers, 1 where the LDS says so
    int per_cu = (int)(kLdsBytes / lds);
    per_cu = per_cu > 2 ? 2 : per_cu;
    const int64_t slots = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(ncol < slots ? ncol : slots);
    kern<<<grid, kThreads, lds, pb::as_stream(stream)>>>(out_d, values_d, ld, counts_d, n, ncol,
                                                        rank_lo_d, rank_hi_d, gamma_d, nq);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
