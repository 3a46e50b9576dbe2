// The posterior modes of a finished nested-sampling run: the rows a resample falls on are linked
// at the scale of their own spacing, the components of the links are the modes, every stored
// point takes the mode of its nearest row, and finish's sums run per mode.  The NumPy statements
// of pyratbay_amd/modes.py (sqdist_host, link_host, assign_host, evidence_host, rows_host) are the
// specification, and every kernel here has their bits; the inputs are rows of the unit cube,
// finite by construction, so nothing here has a rule for NaN.
//
// One sweep serves the distances of all kernels: a thread owns a point, tiles of 32 rows are
// staged in LDS in chunks of 16 parameters, and the thread keeps the 32 partial sums of the tile
// in registers.  The chunks are visited in ascending order, so that every squared distance is the
// left-to-right sum d2 = d2 + t * t of the statement (products and sums round separately: the
// build passes -ffp-contract=off).  FP64 vector arithmetic only: a Gram-matrix form would change
// the bits, and labels flip at the `<= ell2` boundary.  No atomics on doubles; plain launches, no
// allocation, no synchronisation.
#include "pb_common.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxPar = PB_RETRIEVAL_MAX_PARAMS;
constexpr int kMaxRows = PB_NESTED_MAX_LIVE;
constexpr int kMaxKnn = PB_MODES_MAX_KNN;
constexpr int kTileRows = 32;                   // rows per tile: one word of the link matrix
constexpr int kChunk = 16;                      // parameters per chunk
constexpr int kBlock = 256;
constexpr int kKnnBlock = 64;                   // 64 lists of 32 doubles: 16 KiB of LDS
constexpr int kLinkBlock = 64;                  // a few thousand rows: small blocks, and the
constexpr int kLinkSplit = 8;                   // rows split over blockIdx.y, fill the chip
constexpr int kCompBlock = 1024;

struct SweepTile {
    double row[kTileRows][kChunk];
    int32_t flag[kTileRows];                    // the row's label (0 without labels); -1: no row
};

// Every thread's point against the rows jlo .. jhi - 1 (jlo a multiple of 32) of B[nb, nfree], tile
// by tile: use.tile(j0, acc, flag) gets the squared distances to the rows j0 .. j0 + 31 (flag < 0:
// not a row).  Every thread of the block takes part in the staging, with or without a point.
template <int kThreads, class Use>
__device__ __forceinline__ void sweep(const double *__restrict__ A, int64_t i, bool have,
                                      const double *__restrict__ B, int nb, int nfree,
                                      const int32_t *__restrict__ rowlab, SweepTile &s, Use &use,
                                      int jlo = 0, int jhi = 1 << 30)
{
    const bool single = nfree <= kChunk;        // (block-uniform)
    double a[kChunk];
#pragma unroll
    for (int pp = 0; pp < kChunk; pp++)
        a[pp] = (single && have && pp < nfree) ? A[i * nfree + pp] : 0.0;
    nb = nb < jhi ? nb : jhi;
    for (int j0 = jlo; j0 < nb; j0 += kTileRows) {
        double acc[kTileRows];
#pragma unroll
        for (int jj = 0; jj < kTileRows; jj++)
            acc[jj] = 0.0;
        for (int p0 = 0; p0 < nfree; p0 += kChunk) {
            __syncthreads();                    // the tile before this one has been used
            for (int e = threadIdx.x; e < kTileRows * kChunk; e += kThreads) {
                const int jj = e / kChunk, pp = e % kChunk;
                const int j = j0 + jj, p = p0 + pp;
                s.row[jj][pp] = (j < nb && p < nfree) ? B[(int64_t)j * nfree + p] : 0.0;
            }
            if (p0 == 0 && threadIdx.x < kTileRows) {
                const int j = j0 + threadIdx.x;
                s.flag[threadIdx.x] = j < nb ? (rowlab ? rowlab[j] : 0) : -1;
            }
            if (!single) {
#pragma unroll
                for (int pp = 0; pp < kChunk; pp++)
                    a[pp] = (have && p0 + pp < nfree) ? A[i * nfree + p0 + pp] : 0.0;
            }
            __syncthreads();
            const int np = nfree - p0 < kChunk ? nfree - p0 : kChunk;   // (block-uniform)
#pragma unroll
            for (int pp = 0; pp < kChunk; pp++) {
                if (pp < np) {
#pragma unroll
                    for (int jj = 0; jj < kTileRows; jj++) {
                        const double t = a[pp] - s.row[jj][pp];
                        acc[jj] = acc[jj] + t * t;
                    }
                }
            }
        }
        if (have)
            use.tile(j0, acc, s.flag);
    }
}

// ---- sqdist_host --------------------------------------------------------------------------------
struct UseStore {
    double *out;                                // the point's row of d2[na, nb]
    __device__ __forceinline__ void tile(int j0, const double (&acc)[kTileRows],
                                         const int32_t *flag)
    {
#pragma unroll
        for (int jj = 0; jj < kTileRows; jj++)
            if (flag[jj] >= 0)
                out[j0 + jj] = acc[jj];
    }
};

__global__ __launch_bounds__(kBlock) void k_modes_sqdist(
    double *__restrict__ d2, const double *__restrict__ A, const double *__restrict__ B,
    int64_t na, int nb, int nfree)
{
    __shared__ SweepTile s;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    UseStore use{d2 + (i < na ? i : 0) * nb};
    sweep<kBlock>(A, i, i < na, B, nb, nfree, nullptr, s, use);
}

// ---- link_host: the k-th nearest other row ------------------------------------------------------
// The thread's running list of its k smallest distances, ascending, in LDS (entry e of thread t at
// list[e * kKnnBlock + t]); duplicates count.
struct UseNearest {
    double *list;
    int k, count;
    int64_t self;
    __device__ __forceinline__ void tile(int j0, const double (&acc)[kTileRows],
                                         const int32_t *flag)
    {
#pragma unroll
        for (int jj = 0; jj < kTileRows; jj++) {
            const double v = acc[jj];
            if (flag[jj] < 0 || j0 + jj == self)
                continue;
            if (count == k && !(v < list[(k - 1) * kKnnBlock]))
                continue;
            int pos = count < k ? count : k - 1;
            while (pos > 0 && list[(pos - 1) * kKnnBlock] > v) {
                list[pos * kKnnBlock] = list[(pos - 1) * kKnnBlock];
                pos--;
            }
            list[pos * kKnnBlock] = v;
            count = count < k ? count + 1 : k;
        }
    }
};

__global__ __launch_bounds__(kKnnBlock) void k_modes_nearest(
    double *__restrict__ dk, const double *__restrict__ R, int n, int nfree, int k)
{
    __shared__ SweepTile s;
    __shared__ double list[kMaxKnn * kKnnBlock];
    const int64_t i = (int64_t)blockIdx.x * kKnnBlock + threadIdx.x;
    UseNearest use{list + threadIdx.x, k, 0, i};
    sweep<kKnnBlock>(R, i, i < n, R, n, nfree, nullptr, s, use);
    if (i < n)
        dk[i] = use.count == k ? list[(k - 1) * kKnnBlock + threadIdx.x] : HUGE_VAL;
}

// One block: ell2 = link2 * max dk.
__global__ __launch_bounds__(kBlock) void k_modes_ell2(
    double *__restrict__ ell2, const double *__restrict__ dk, int n, double link2)
{
    __shared__ double part[kBlock];
    double m = -HUGE_VAL;
    for (int i = threadIdx.x; i < n; i += kBlock)
        m = fmax(m, dk[i]);
    part[threadIdx.x] = m;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0)
        ell2[0] = link2 * part[0];
}

// ---- link_host: the links as a bit matrix -------------------------------------------------------
// bits[n, ceil(n / 32)]: bit j % 32 of word j / 32 of row i is set iff i != j and d2 <= ell2;
// 2 MiB at 4096 rows.
struct UseLinks {
    uint32_t *words;
    double ell2;
    int64_t self;
    __device__ __forceinline__ void tile(int j0, const double (&acc)[kTileRows],
                                         const int32_t *flag)
    {
        uint32_t word = 0;
#pragma unroll
        for (int jj = 0; jj < kTileRows; jj++)
            if (flag[jj] >= 0 && j0 + jj != self && acc[jj] <= ell2)
                word |= 1u << jj;
        words[j0 / kTileRows] = word;
    }
};

__global__ __launch_bounds__(kLinkBlock) void k_modes_links(
    uint32_t *__restrict__ bits, const double *__restrict__ ell2, const double *__restrict__ R,
    int n, int nfree)
{
    __shared__ SweepTile s;
    const int64_t i = (int64_t)blockIdx.x * kLinkBlock + threadIdx.x;
    const int nwords = (n + kTileRows - 1) / kTileRows;
    // blockIdx.y takes its share of the words of every row
    const int per = (nwords + kLinkSplit - 1) / kLinkSplit;
    const int jlo = (int)blockIdx.y * per * kTileRows;
    UseLinks use{bits + (i < n ? i : 0) * nwords, ell2[0], i};
    sweep<kLinkBlock>(R, i, i < n, R, n, nfree, nullptr, s, use, jlo, jlo + per * kTileRows);
}

// ---- link_host: components, canonical order, labels ---------------------------------------------
// One block, the labels in LDS.  lab[i] starts at i and only falls, always to a row of the same
// component.  A pass: one wavefront per row takes the smallest label among the row and its links
// and hooks it onto the row and onto the row its label names (integer atomics); then every row
// jumps to the end of its chain of labels.  Passes repeat until one changes nothing: then lab is
// constant over every component and names its smallest row, whatever the order of the updates.
// Then the sizes, the canonical order by counting (size descending, ties to the smaller row) and
// the labels.  No host loop, nothing read back.
__global__ __launch_bounds__(kCompBlock) void k_modes_components(
    int32_t *__restrict__ labels, int32_t *__restrict__ nmodes, const uint32_t *__restrict__ bits,
    int n, int min_mode, int max_modes)
{
    __shared__ int32_t lab_s[kMaxRows], size_s[kMaxRows], mode_s[kMaxRows];
    __shared__ int changed, count;
    volatile int32_t *lab = lab_s;
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const int nwords = (n + kTileRows - 1) / kTileRows;
    for (int i = t; i < n; i += kCompBlock) {
        lab_s[i] = i;
        size_s[i] = 0;
    }
    if (t == 0)
        count = 0;
    __syncthreads();
    for (;;) {
        if (t == 0)
            changed = 0;
        __syncthreads();
        for (int i = wave; i < n; i += kCompBlock / kWave) {        // (wave-uniform)
            const int own = __shfl((int)lab[i], 0, kWave);
            int m = own;
            for (int w = lane; w < nwords; w += kWave) {
                uint32_t word = bits[(int64_t)i * nwords + w];
                while (word) {
                    const int j = w * kTileRows + __ffs(word) - 1;
                    word &= word - 1;
                    if (j < n)
                        m = min(m, (int)lab[j]);
                }
            }
            for (int off = kWave / 2; off > 0; off >>= 1)
                m = min(m, __shfl_xor(m, off, kWave));
            if (lane == 0 && m < own) {
                atomicMin(&lab_s[own], m);
                atomicMin(&lab_s[i], m);
                changed = 1;
            }
        }
        __syncthreads();
        for (int i = t; i < n; i += kCompBlock) {
            int l = lab[i];
            for (int up = lab[l]; up != l; up = lab[l])
                l = up;
            lab[i] = l;
        }
        __syncthreads();
        const int again = changed;
        __syncthreads();
        if (!again)
            break;
    }
    for (int i = t; i < n; i += kCompBlock)
        atomicAdd(&size_s[lab_s[i]], 1);
    __syncthreads();
    for (int i = t; i < n; i += kCompBlock) {
        if (lab_s[i] != i)
            continue;
        const int mine = size_s[i];
        int q = 0;
        for (int j = 0; j < n; j++)
            q += (lab_s[j] == j && (size_s[j] > mine || (size_s[j] == mine && j < i))) ? 1 : 0;
        const bool is_mode = q == 0 || (mine >= min_mode && q < max_modes);
        mode_s[i] = is_mode ? q : -1;
        if (is_mode)
            atomicMax(&count, q + 1);
    }
    __syncthreads();
    for (int i = t; i < n; i += kCompBlock)
        labels[i] = mode_s[lab_s[i]];
    if (t == 0)
        nmodes[0] = count;
}

// ---- assign_host --------------------------------------------------------------------------------
// The minimum over (d2, row) among the labelled rows: the rows come in ascending order and only a
// strictly smaller distance replaces the best one.
struct UseClosest {
    double best;
    int32_t label;
    __device__ __forceinline__ void tile(int j0, const double (&acc)[kTileRows],
                                         const int32_t *flag)
    {
#pragma unroll
        for (int jj = 0; jj < kTileRows; jj++)
            if (flag[jj] >= 0 && acc[jj] < best) {
                best = acc[jj];
                label = flag[jj];
            }
    }
};

__global__ __launch_bounds__(kBlock) void k_modes_assign(
    int32_t *__restrict__ mode, const double *__restrict__ P, const double *__restrict__ R,
    const int32_t *__restrict__ labels, int64_t np, int n, int nfree)
{
    __shared__ SweepTile s;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    UseClosest use{HUGE_VAL, -1};
    sweep<kBlock>(P, i, i < np, R, n, nfree, labels, s, use);
    if (i < np)
        mode[i] = use.label;
}

// ---- rows_host ----------------------------------------------------------------------------------
// One block: the indices with counts > 0, ascending, by chunks of consecutive indices; the first
// `cap` of them are written, all are counted.
__global__ __launch_bounds__(kBlock) void k_modes_rows(
    int64_t *__restrict__ rows, int64_t *__restrict__ nrows, const int64_t *__restrict__ counts,
    int64_t n, int64_t cap)
{
    __shared__ int64_t before[kBlock];
    const int t = threadIdx.x;
    const int64_t per = (n + kBlock - 1) / kBlock;
    const int64_t lo = t * per < n ? t * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    int64_t mine = 0;
    for (int64_t i = lo; i < hi; i++)
        mine += counts[i] > 0 ? 1 : 0;
    before[t] = mine;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int c = 0; c < kBlock; c++) {
            const int64_t here = before[c];
            before[c] = run;
            run += here;
        }
        nrows[0] = run;
    }
    __syncthreads();
    int64_t at = before[t];
    for (int64_t i = lo; i < hi; i++)
        if (counts[i] > 0) {
            if (at < cap)
                rows[at] = i;
            at++;
        }
}

// ---- evidence_host ------------------------------------------------------------------------------
// One block per mode: k_nested_finish's sums over the mode's rows, every other row a zero in its
// place, in the same 256 chunks of consecutive rows.
__global__ __launch_bounds__(kBlock) void k_modes_evidence(
    double *__restrict__ ln_z_m, double *__restrict__ info_m, double *__restrict__ fraction_m,
    const double *__restrict__ logw, const double *__restrict__ logl,
    const int32_t *__restrict__ mode, const double *__restrict__ ln_z, int64_t n)
{
    __shared__ double part[kBlock], hpart[kBlock];
    const int t = threadIdx.x, c = blockIdx.x;
    double m = -HUGE_VAL;
    for (int64_t i = t; i < n; i += kBlock)
        if (mode[i] == c && logw[i] > -HUGE_VAL)
            m = fmax(m, logw[i]);
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
    double sum = 0.0, hsum = 0.0;
    for (int64_t i = lo; i < hi; i++) {
        const double e = (mode[i] == c && logw[i] > -HUGE_VAL) ? exp(logw[i] - m) : 0.0;
        sum = sum + e;
        hsum = hsum + (e > 0.0 ? e * logl[i] : 0.0);
    }
    part[t] = sum;
    hpart[t] = hsum;
    __syncthreads();
    if (t != 0)
        return;
    double run = 0.0, hrun = 0.0;
    for (int k = 0; k < kBlock; k++) {
        run = run + part[k];
        hrun = hrun + hpart[k];
    }
    const double z = m + log(run);
    ln_z_m[c] = z;
    info_m[c] = hrun / run - z;
    fraction_m[c] = exp(z - ln_z[0]);
}

}  // namespace

#define PB_MODES_SHAPE(name, n, nfree)                                                          \
    do {                                                                                        \
        PB_REQUIRE((nfree) >= 1 && (nfree) <= kMaxPar, name ": %d free parameters: 1 to %d",    \
                   (nfree), kMaxPar);                                                           \
        PB_REQUIRE((n) >= 1 && (n) <= kMaxRows, name ": %d rows: 1 to %d", (n), kMaxRows);      \
    } while (0)

extern "C" {

int pb_modes_sqdist(double *d2_d, const double *a_d, const double *b_d, int64_t na, int nb,
                    int nfree, void *stream)
{
    PB_MODES_SHAPE("pb_modes_sqdist", nb, nfree);
    PB_REQUIRE(na >= 0 && na <= ((int64_t)1 << 31) - kBlock, "pb_modes_sqdist: bad shape");
    PB_REQUIRE(d2_d && a_d && b_d, "pb_modes_sqdist: null pointer");
    if (na == 0)
        return PB_OK;
    k_modes_sqdist<<<pb::div_up(na, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        d2_d, a_d, b_d, na, nb, nfree);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_modes_link(int32_t *labels_d, int32_t *nmodes_d, double *ell2_d, double *dk_d,
                  int32_t *bits_d, const double *r_d, int n, int nfree, int knn, double link,
                  int min_mode, int max_modes, void *stream)
{
    PB_MODES_SHAPE("pb_modes_link", n, nfree);
    PB_REQUIRE(n >= 2, "pb_modes_link: %d rows: at least 2", n);
    PB_REQUIRE(knn >= 1 && knn <= kMaxKnn, "pb_modes_link: knn = %d: 1 to %d", knn, kMaxKnn);
    PB_REQUIRE(max_modes >= 1, "pb_modes_link: max_modes = %d: at least 1", max_modes);
    PB_REQUIRE(labels_d && nmodes_d && ell2_d && dk_d && bits_d && r_d,
               "pb_modes_link: null pointer");
    hipStream_t s = pb::as_stream(stream);
    const int k = knn < n - 1 ? knn : n - 1;
    k_modes_nearest<<<pb::div_up(n, kKnnBlock), kKnnBlock, 0, s>>>(dk_d, r_d, n, nfree, k);
    PB_LAUNCH_CHECK();
    k_modes_ell2<<<1, kBlock, 0, s>>>(ell2_d, dk_d, n, link * link);
    PB_LAUNCH_CHECK();
    k_modes_links<<<dim3(pb::div_up(n, kLinkBlock), kLinkSplit), kLinkBlock, 0, s>>>(
        (uint32_t *)bits_d, ell2_d, r_d, n, nfree);
    PB_LAUNCH_CHECK();
    k_modes_components<<<1, kCompBlock, 0, s>>>(labels_d, nmodes_d, (const uint32_t *)bits_d, n,
                                                min_mode, max_modes);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_modes_assign(int32_t *mode_d, const double *p_d, const double *r_d,
                    const int32_t *labels_d, int64_t np, int n, int nfree, void *stream)
{
    PB_MODES_SHAPE("pb_modes_assign", n, nfree);
    PB_REQUIRE(np >= 0 && np <= ((int64_t)1 << 31) - kBlock, "pb_modes_assign: bad shape");
    PB_REQUIRE(mode_d && p_d && r_d && labels_d, "pb_modes_assign: null pointer");
    if (np == 0)
        return PB_OK;
    k_modes_assign<<<pb::div_up(np, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        mode_d, p_d, r_d, labels_d, np, n, nfree);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_modes_rows(int64_t *rows_d, int64_t *nrows_d, const int64_t *counts_d, int64_t n,
                  int64_t cap, void *stream)
{
    PB_REQUIRE(n >= 1 && cap >= 0, "pb_modes_rows: bad shape");
    PB_REQUIRE(rows_d && nrows_d && counts_d, "pb_modes_rows: null pointer");
    k_modes_rows<<<1, kBlock, 0, pb::as_stream(stream)>>>(rows_d, nrows_d, counts_d, n, cap);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_modes_evidence(double *ln_z_m_d, double *info_m_d, double *fraction_m_d,
                      const double *logw_d, const double *logl_d, const int32_t *mode_d,
                      const double *ln_z_d, int64_t n, int nmodes, void *stream)
{
    PB_REQUIRE(n >= 1 && nmodes >= 0 && nmodes <= kMaxRows, "pb_modes_evidence: bad shape");
    PB_REQUIRE(ln_z_m_d && info_m_d && fraction_m_d && logw_d && logl_d && mode_d && ln_z_d,
               "pb_modes_evidence: null pointer");
    if (nmodes == 0)
        return PB_OK;
    k_modes_evidence<<<nmodes, kBlock, 0, pb::as_stream(stream)>>>(
        ln_z_m_d, info_m_d, fraction_m_d, logw_d, logl_d, mode_d, ln_z_d, n);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
