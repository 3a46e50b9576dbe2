// Walker-batched retrieval path, the transit pass: ray paths, optical depth with the reference's
// early exit and the transmission integral for a batch of atmospheres in one launch
// (atmosphere/atmosphere.py:782-802, opacity/optic_depth.py:103-112 -> src_c/_trapezoid.c:238-276,
// spectrum/radiative_transfer.py:57-71).  The overview of the batch is in pb_interp.hip.
//
//   k_transit_path        raypath[w][r(r-1)/2 + i] from radius[w][L]
//   k_path_blocks         ray paths re-laid per block of rows for scalar loads
//   k_transit_fused       one column per thread: depth, ideep and spectrum, any shape
//   k_transit_pair        two columns per thread: the retrieval batch (spectrum only)
//   k_path_qblocks        ray paths as the 16 x 4 blocks of the matrix-core operand
//   k_transit_mfma_rows   the retrieval batch on the matrix cores, row tile by row tile
//
// Which of them a call uses is plan_transit()'s decision; pb_transit_fused_launch() launches what
// it chose.
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <type_traits>

#include "pb_common.h"
#include "pb_transit.h"

using namespace pbt;

namespace {

constexpr int kBlock = 256;

using pb::TileLimit;              // (pb_common.h; the layers nobody reads: pb_interp.hip)
using pb::uniform_i32;

// ---------------------------------------------------------------------------
// atmosphere.transit_path: path_r[i] = sqrt(rad_i^2 - rad_r^2) - sqrt(rad_{i+1}^2 - rad_r^2),
// rad = radius[itop:], packed lower triangle (row r has r entries from r(r-1)/2).  One multiply per
// square; the reference's pow(x, 2) is 1 ulp off x*x for 0.09 % of values: those rows agree to 1e-12.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_transit_path(double *raypath, const double *radius,
                                                         int itop, int nlayers, int64_t npath)
{
    const int w = blockIdx.y;
    const double *rad = radius + (int64_t)w * nlayers + itop;
    double *out = raypath + (int64_t)w * npath;
    const int nrow = nlayers - itop;
    for (int r = blockIdx.x; r < nrow; r += gridDim.x) {
        const double rr = rad[r] * rad[r];
        for (int i = threadIdx.x; i < r; i += kBlock) {
            const double a = rad[i] * rad[i] - rr;
            const double b = rad[i + 1] * rad[i + 1] - rr;
            out[((int64_t)r * (r - 1)) / 2 + i] = sqrt(a) - sqrt(b);
        }
    }
}

// Ray paths re-laid for the fused kernel: for every block of kRows impact parameters the segments
// [i][row], zero where segment >= row -- contiguous per (block, segment), so that the kernel can
// take them with wide SCALAR loads (they are wave-uniform) and feed v_fma_f64 from SGPRs.
__global__ __launch_bounds__(kBlock) void k_path_blocks(double *blocked, const double *raypath,
                                                        int64_t npath, int64_t nblocked, int rows,
                                                        int nimpact)
{
    const int w = blockIdx.y;
    const double *path = raypath + (int64_t)w * npath;
    double *out = blocked + (int64_t)w * nblocked;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nblocked;
         e += (int64_t)gridDim.x * kBlock) {
        // block b starts at rows * sum_{b'<b} nseg_b', nseg_b = min(rows*b + rows, nimpact) - 1
        int b = 0;
        int64_t off = 0;
        for (;;) {
            const int64_t n = (int64_t)max(min(rows * b + rows, nimpact) - 1, 0) * rows;
            if (e < off + n)
                break;
            off += n;
            b++;
        }
        const int i = (int)((e - off) / rows), k = (int)((e - off) % rows);
        const int r = rows * b + k;
        out[e] = (r < nimpact && i < r) ? path[((int64_t)r * (r - 1)) / 2 + i] : 0.0;
    }
}

// ---------------------------------------------------------------------------
// Transit optical depth + transmission, one pass per column (optic_depth.py:103-112 with the
// early exit of _trapezoid.c:259-273, radiative_transfer.py:57-71 incl. the cloud deck).
// thread = column (x walker); the impact parameters are taken kRows at a time: for one block of
// rows the column of ec is streamed from its top (coalesced over columns; the re-reads of
// later blocks come from L2 / the Infinity Cache), the kRows running sums stay in registers and
// the ray-path segments of the block sit in LDS ([segment][row], zero where segment >= row, so one
// predicate-free loop serves all rows with the reference's products and additions).  After each
// block its rows are examined in order: pb::exp_s(-tau)*r joins the trapezoid, the first tau above
// maxdepth ends the column -- later blocks are not computed at all, which is where the time
// of the two-kernel form went (every row of every column, then a second pass to find the exit).
// depth and ideep are optional outputs (a retrieval needs neither).
// ---------------------------------------------------------------------------
using pb::deck_integrand;         // (pb_common.h)

// tau += path*s is the reference's product-then-sum (two roundings); the retrieval batch
// (spectrum only) runs k_transit_pair, which fuses them: results equal to ~1e-16 relative.
template <int kRows, bool kScalarPath>
__global__ __launch_bounds__(kBlock) void k_transit_fused(
    double *depth, int32_t *ideep, double *spectrum, const double *ec, const double *raypath,
    const double *radius, int64_t npath, double rstar, int itop, int ibottom, double maxdepth,
    int nlayers, int nwave, int deck_row, double rsurf)
{
    // kScalarPath: raypath is the blocked layout of k_path_blocks (npath = its length per
    // walker), read through the constant address space = scalar loads; else the packed lower
    // triangle, staged per block in LDS
    extern __shared__ __align__(16) double s_path[];      // [segment][kRows]
    const int w = blockIdx.y;
    const int col = blockIdx.x * kBlock + threadIdx.x;
    const bool active = col < nwave;
    const int64_t plane = (int64_t)nlayers * nwave;
    ec += (int64_t)w * plane;
    if (depth)
        depth += (int64_t)w * plane;
    const double *path = raypath ? raypath + (int64_t)w * npath : nullptr;
    // the walker's radii are wave-uniform: scalar loads through the constant address space
    typedef const double __attribute__((address_space(4))) *crad_t;
    const crad_t rad = (crad_t)(unsigned long long)(radius ? radius + (int64_t)w * nlayers : nullptr);
    const int nimpact = min(ibottom, nlayers) - itop;     // rows 0..nimpact-1 are evaluated
    const double *src = ec + (int64_t)itop * nwave + (active ? col : 0);

    int stop = -1;
    double acc = 0.0, fprev = 0.0, rprev = 0.0;
    if (depth && active)
        for (int r = 0; r < itop; r++)
            depth[(int64_t)r * nwave + col] = 0.0;
    int rdone = 0;                       // rows examined so far (uniform)
    int64_t boff = 0;                    // start of the current block in the blocked path layout
    for (int rb = 0; rb < nimpact; rb += kRows) {
        // every column of the workgroup has met its exit: nothing left to compute
        if (__syncthreads_count(active && stop < 0) == 0)
            break;
        const int rlast = min(rb + kRows, nimpact) - 1;
        const int nseg = max(rlast, 0);
        if (!kScalarPath) {
            for (int e = threadIdx.x; e < nseg * kRows; e += kBlock) {
                const int i = e / kRows, k = e % kRows;
                const int r = rb + k;
                s_path[e] = (r <= rlast && i < r) ? path[((int64_t)r * (r - 1)) / 2 + i] : 0.0;
            }
            __syncthreads();
        }
        rdone = rlast + 1;
        if (!active) {
            boff += (int64_t)nseg * kRows;
            continue;
        }
        if (stop >= 0) {
            // below the first crossing the reference leaves zeros
            if (depth)
                for (int r = rb; r <= rlast; r++)
                    depth[(int64_t)(itop + r) * nwave + col] = 0.0;
            boff += (int64_t)nseg * kRows;
            continue;
        }
        double tau[kRows];
#pragma unroll
        for (int k = 0; k < kRows; k++)
            tau[k] = 0.0;
        if (nseg > 0) {
            double prev = src[0];
            if (kScalarPath) {
                typedef const double __attribute__((address_space(4))) *cpath_t;
                const cpath_t pb_ = (cpath_t)(unsigned long long)(path + boff);
#pragma unroll 2
                for (int i = 0; i < nseg; i++) {
                    const double next = src[(int64_t)(i + 1) * nwave];
                    const double s = next + prev;
                    prev = next;
                    double pv[kRows];                           // wave-uniform: scalar loads
#pragma unroll
                    for (int k = 0; k < kRows; k++)
                        pv[k] = pb_[i * kRows + k];
#pragma unroll
                    for (int k = 0; k < kRows; k++)
                        tau[k] = tau[k] + pv[k] * s;
                }
            } else {
#pragma unroll 4
                for (int i = 0; i < nseg; i++) {
                    const double next = src[(int64_t)(i + 1) * nwave];
                    const double s = next + prev;
                    prev = next;
                    const double *pk = s_path + i * kRows;      // LDS broadcast reads
#pragma unroll
                    for (int k = 0; k < kRows; k++)
                        tau[k] += pk[k] * s;
                }
            }
        }
        boff += (int64_t)nseg * kRows;
#pragma unroll
        for (int k = 0; k < kRows; k++) {
            const int r = rb + k;
            if (r <= rlast) {
                double t = tau[k];
                if (stop < 0) {
                    if (spectrum) {
                        const double rr = rad[itop + r];
                        double f = pb::exp_s(-t) * rr;
                        if (r > 0 && r == deck_row) {
                            f = deck_integrand(fprev, f, rprev, rr, rsurf);
                            acc += (rsurf - rprev) * (fprev + f);
                        } else if (r > 0) {
                            acc += (rr - rprev) * (fprev + f);
                        }
                        fprev = f;
                        rprev = rr;
                    }
                    if (t > maxdepth)
                        stop = r;
                } else {
                    t = 0.0;
                }
                if (depth)
                    depth[(int64_t)(itop + r) * nwave + col] = t;
            }
        }
    }
    if (!active)
        return;
    if (depth)
        for (int r = max(rdone, 0); r < nlayers - itop; r++)
            depth[(int64_t)(itop + r) * nwave + col] = 0.0;   // rows never reached, rows >= ibottom
    // ideep[ideep<0] = r with r the last loop value (itop if the loop is empty)
    const int last = nimpact > 0 ? itop + nimpact - 1 : itop;
    if (ideep)
        ideep[(int64_t)w * nwave + col] = stop >= 0 ? itop + stop : last;
    if (spectrum) {
        const double rtop = rad[itop];
        spectrum[(int64_t)w * nwave + col] = (rtop * rtop + 2 * (acc * 0.5)) / (rstar * rstar);
    }
}

// ---------------------------------------------------------------------------
// The retrieval batch (spectrum only, no cloud deck): the same pass with TWO columns per thread,
// so that every ray-path value fetched by a scalar load feeds two fused multiply-adds -- the
// scalar cache cannot hold the ray paths of the few walkers a CU works on at once (30 KB each),
// and with one column per thread the waits for those loads are half of the kernel's time.
// ---------------------------------------------------------------------------
template <int kRows>
__global__ __launch_bounds__(kBlock) void k_transit_pair(
    double *spectrum, const double *ec, const double *blocked, const double *radius, int64_t plen,
    double rstar, int itop, int ibottom, double maxdepth, int nlayers, int nwave)
{
    const int w = blockIdx.y;
    const int col[2] = {(int)(blockIdx.x * 2 * kBlock + threadIdx.x),
                        (int)(blockIdx.x * 2 * kBlock + kBlock + threadIdx.x)};
    const bool active[2] = {col[0] < nwave, col[1] < nwave};
    const int64_t plane = (int64_t)nlayers * nwave;
    ec += (int64_t)w * plane;
    typedef const double __attribute__((address_space(4))) *cdbl_t;
    const cdbl_t rad = (cdbl_t)(unsigned long long)(radius + (int64_t)w * nlayers);
    const cdbl_t path = (cdbl_t)(unsigned long long)(blocked + (int64_t)w * plen);
    const int nimpact = min(ibottom, nlayers) - itop;
    const double *src[2] = {ec + (int64_t)itop * nwave + (active[0] ? col[0] : 0),
                            ec + (int64_t)itop * nwave + (active[1] ? col[1] : 0)};
    int stop[2] = {-1, -1};
    double acc[2] = {0.0, 0.0}, fprev[2] = {0.0, 0.0};
    int64_t boff = 0;
    for (int rb = 0; rb < nimpact; rb += kRows) {
        if (__syncthreads_count((active[0] && stop[0] < 0) || (active[1] && stop[1] < 0)) == 0)
            break;
        const int rlast = min(rb + kRows, nimpact) - 1;
        const int nseg = max(rlast, 0);
        double tau[2][kRows];
#pragma unroll
        for (int k = 0; k < kRows; k++)
            tau[0][k] = tau[1][k] = 0.0;
        if (nseg > 0) {
            double prev0 = src[0][0], prev1 = src[1][0];
            const cdbl_t pb_ = path + boff;
            // rows of ec are fetched kAhead at a time, one group ahead of the sums that use them
            // (a wavefront then keeps 2 x kAhead row loads in flight: the stream comes from HBM)
            constexpr int kAhead = 4;
            double nx0[kAhead], nx1[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; j++) {
                const int64_t row = (int64_t)min(j + 1, nseg) * nwave;
                nx0[j] = src[0][row];
                nx1[j] = src[1][row];
            }
            for (int i0 = 0; i0 < nseg; i0 += kAhead) {
                double c0[kAhead], c1[kAhead];
#pragma unroll
                for (int j = 0; j < kAhead; j++) {
                    c0[j] = nx0[j];
                    c1[j] = nx1[j];
                }
#pragma unroll
                for (int j = 0; j < kAhead; j++) {
                    const int64_t row = (int64_t)min(i0 + kAhead + j + 1, nseg) * nwave;
                    nx0[j] = src[0][row];
                    nx1[j] = src[1][row];
                }
#pragma unroll
                for (int j = 0; j < kAhead; j++) {
                    const int i = i0 + j;
                    if (i < nseg) {                             // uniform
                        const double s0 = c0[j] + prev0, s1 = c1[j] + prev1;
                        prev0 = c0[j];
                        prev1 = c1[j];
                        double pv[kRows];                       // wave-uniform: scalar loads
#pragma unroll
                        for (int k = 0; k < kRows; k++)
                            pv[k] = pb_[i * kRows + k];
#pragma unroll
                        for (int k = 0; k < kRows; k++) {
                            tau[0][k] = fma(pv[k], s0, tau[0][k]);
                            tau[1][k] = fma(pv[k], s1, tau[1][k]);
                        }
                    }
                }
            }
        }
        boff += (int64_t)nseg * kRows;
#pragma unroll
        for (int c = 0; c < 2; c++) {
#pragma unroll
            for (int k = 0; k < kRows; k++) {
                const int r = rb + k;
                if (r <= rlast && active[c] && stop[c] < 0) {
                    const double t = tau[c][k];
                    const double rr = rad[itop + r];
                    const double f = pb::exp_s(-t) * rr;
                    if (r > 0)
                        acc[c] += (rr - rad[itop + r - 1]) * (fprev[c] + f);
                    fprev[c] = f;
                    if (t > maxdepth)
                        stop[c] = r;
                }
            }
        }
    }
    const double rtop = rad[itop];
#pragma unroll
    for (int c = 0; c < 2; c++)
        if (active[c])
            spectrum[(int64_t)w * nwave + col[c]] =
                (rtop * rtop + 2 * (acc[c] * 0.5)) / (rstar * rstar);
}

// ---------------------------------------------------------------------------
// The retrieval batch on the matrix cores.  Per walker the optical depths are ONE triangular
// matrix product shared by all of its columns,
//     tau[r][col] = sum_{j<=r} Q[r][j] * ec[itop + j][col],   Q[r][j] = P[r][j] + P[r][j-1]
// (P = the ray paths of optic_depth.py:103-112: sum_i P[r][i] (ec[i+1] + ec[i]) regrouped by
// layer), an 80 x 80 lower-triangular Q against an 80 x 1e5 block of ec at C5's shape.
// v_mfma_f64_16x16x4_f64: A = a 16-row x 4-layer block of Q (one double per lane, from LDS, laid
// out in lane order by k_path_qblocks), B = 4 layers x 16 columns of ec (one double per lane,
// straight from global memory: lane = (layer l>>4, column l&15), 128-byte runs), C = 16 rows x 16
// columns of tau (4 doubles per lane).  A wavefront owns NT column tiles and all MT row tiles:
// NT x MT accumulators stay in registers while ec streams past ONCE (the vector form re-read
// every column once per block of 16 rows: 3x at 80 layers), and of the MT x 4MT blocks of Q only
// the 2MT^2 + 2MT on or below the diagonal are multiplied (60 of 100 at 80 layers).
// The epilogue -- exp(-tau) r, first crossing of maxdepth, trapezoid over the rows
// (radiative_transfer.py:57-71) -- runs on the accumulator layout: lane (q = l>>4, n = l&15) holds
// the rows 16m + 4j + q of column n; the previous row's integrand comes from the lane 16 below
// (one cross-lane move per row), the first crossing and the sums are combined over the four lanes
// of a column.  Sums of a column are added in a different order than the reference's loop:
// spectra agree to ~1e-15 relative with the vector form, not bit for bit.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_path_qblocks(double *out, const double *raypath,
                                                         int64_t npath, int nblk, int nimpact)
{
    const int w = blockIdx.y;
    const double *path = raypath + (int64_t)w * npath;
    double *o = out + (int64_t)w * nblk * 64;
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < nblk * 64; e += gridDim.x * kBlock) {
        const int blk = e >> 6, l = e & 63;
        int m = 0;
        while (qblocks(m + 1) <= blk)
            m++;
        const int ks = blk - qblocks(m);
        const int r = 16 * m + (l & 15), j = 4 * ks + (l >> 4);
        double v = 0.0;
        if (r >= 1 && r < nimpact && j <= r) {
            const int64_t base = ((int64_t)r * (r - 1)) / 2;
            if (j < r)
                v = path[base + j];
            if (j >= 1)
                v += path[base + j - 1];
        }
        o[e] = v;
    }
}

#ifdef PB_EXPERIMENTS   // the layers-outer matrix kernel of round 3 (replaced by k_transit_mfma_rows)
// A wavefront owns 32 columns = two 16-column tiles (the even and the odd columns of its range:
// one 16-byte load per lane fetches both) and all MT row tiles: 2 x MT accumulators stay in
// registers while the layers stream past once, four K-steps (16 layers) in flight ahead of the
// four being multiplied.  The loads carry no branch (rows beyond the last layer and columns beyond
// the grid read a clamped address: their Q entries are zero, their results unused): behind a
// divergent `if` the compiler drains every load (s_waitcnt vmcnt(0)) before it issues the next.
template <int MT, int WPS, int TB>
__global__ __launch_bounds__(TB, WPS) void k_transit_mfma(
    double *spectrum, const double *ec, const double *qblk, const double *radius, int nblk,
    double rstar, int itop, int ibottom, double maxdepth, int nlayers, int nwave)
{
    extern __shared__ __align__(16) double s_q[];         // [nblk][64] | rad[16 MT]
    const int w = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nimpact = min(ibottom, nlayers) - itop;
    double *s_rad = s_q + (size_t)nblk * 64;
    {
        stage_qblocks<MT, TB>(s_q, qblk + (int64_t)w * nblk * 64, tid);
        for (int r = tid; r < 16 * MT; r += TB)
            s_rad[r] = r < nimpact ? radius[(int64_t)w * nlayers + itop + r] : 0.0;
    }
    __syncthreads();
    const int c0 = (blockIdx.x * (TB / 64) + wave) * 32;
    if (c0 >= nwave)
        return;                                           // (after the only barrier)
    const int kq = lane >> 4, n = lane & 15;
    const int col0 = c0 + 2 * n;                          // tile 0: even columns, tile 1: odd ones
    const bool ok[2] = {col0 < nwave, col0 + 1 < nwave};
    const int cpair = max(min(col0, nwave - 2), 0);       // first column of the pair I load
    const bool second = col0 != cpair;                    // my column 0 is the pair's second one
    const double *src = ec + ((int64_t)w * nlayers + itop) * nwave + cpair;
    const int KS = (nimpact + 3) / 4;
    v4d C[2][MT];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int m = 0; m < MT; m++)
            C[t][m] = v4d{0.0, 0.0, 0.0, 0.0};
    double bcur[4][2], bnxt[4][2];
    auto loadb = [&](int mb, double (&b)[4][2]) {         // (the launcher guarantees nwave >= 2)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            const int j = min(4 * (4 * mb + kk) + kq, nimpact - 1);
            const d2u v = *reinterpret_cast<const d2u *>(src + (int64_t)j * nwave);
            b[kk][0] = second ? v.y : v.x;
            b[kk][1] = v.y;
        }
    };
    loadb(0, bcur);
    const double *sq = s_q + lane;
#pragma unroll
    for (int mb = 0; mb < MT; mb++) {
        if (4 * mb < KS) {                                // uniform
            if (mb + 1 < MT)
                loadb(mb + 1, bnxt);
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const int ks = 4 * mb + kk;
#pragma unroll
                for (int m = mb; m < MT; m++) {
                    const double a = sq[(qblocks(m) + ks) * 64];
                    C[0][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bcur[kk][0], C[0][m], 0, 0, 0);
                    C[1][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bcur[kk][1], C[1][m], 0, 0, 0);
                }
            }
            if (mb + 1 < MT) {
#pragma unroll
                for (int kk = 0; kk < 4; kk++) {
                    bcur[kk][0] = bnxt[kk][0];
                    bcur[kk][1] = bnxt[kk][1];
                }
            }
        }
    }
    mfma_transit_epilogue<MT>(C, s_rad, spectrum + (int64_t)w * nwave, col0, ok, lane, nimpact,
                              maxdepth, rstar);
}

#endif  // PB_EXPERIMENTS

// The same products ROW TILE BY ROW TILE, with the reference's early exit at tile granularity
// (_trapezoid.c:259-273: a column is finished at the first row whose optical depth exceeds
// maxdepth).  Row tile m needs the layers 0 .. 16m + 15 only, so the B operands stay in registers
// (2 doubles per K-step and lane: 80 registers at 80 layers) while ONE row tile's accumulators are
// live; its rows go through the epilogue at once (carry, sums and first crossing kept across
// tiles), and when every column of the wavefront has crossed, the remaining tiles -- their products
// AND the loads of their layers, which are issued one tile ahead -- are skipped.  Per column the
// products, their order and the epilogue's arithmetic are those of k_transit_mfma: same bits.
// Columns that cross at similar rows must sit together for the exit to happen: the caller orders
// the columns (TableSpectrum.column_order) and passes `scatter`, the grid index of each column.
template <int B, int E, class F>
__device__ __forceinline__ void static_for_rows(F &&f)
{
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for_rows<B + 1, E>(f);
    }
}

// pb::exp_s of four values at once, cut into 15 slices of four independent instructions each (the
// same operations in the same order per value: same bits), so that the slices of one column tile's
// epilogue can be issued between the matrix products of the other (k_transit_mfma_rows).
struct Exp4 {
    double x[4], n[4], r[4], p[4];
};
constexpr int kExp4Slices = 15;
template <int S>
__device__ __forceinline__ void exp4_slice(Exp4 &e)
{
    using pb::sgpr_const;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if constexpr (S == 0)
            e.n[j] = rint(e.x[j] * sgpr_const(0x1.71547652b82fep+0));
        else if constexpr (S == 1)
            e.r[j] = fma(e.n[j], sgpr_const(-0x1.62e42fefa39efp-1), e.x[j]);
        else if constexpr (S == 2)
            e.r[j] = fma(sgpr_const(-0x1.abc9e3b39803fp-56), e.n[j], e.r[j]);
        else if constexpr (S == 3)
            e.p[j] = fma(sgpr_const(0x1.ade156a5dcb37p-26), e.r[j], sgpr_const(0x1.28af3fca7ab0cp-22));
        else if constexpr (S == 4)
            e.p[j] = fma(e.r[j], e.p[j], sgpr_const(0x1.71dee623fde64p-19));
        else if constexpr (S == 5)
            e.p[j] = fma(e.r[j], e.p[j], sgpr_const(0x1.a01997c89e6b0p-16));
        else if constexpr (S == 6)
            e.p[j] = fma(e.r[j], e.p[j], sgpr_const(0x1.a01a014761f6ep-13));
        else if constexpr (S == 7)
            e.p[j] = fma(e.r[j], e.p[j], sgpr_const(0x1.6c16c1852b7b0p-10));
        else if constexpr (S == 8)
            e.p[j] = fma(e.r[j], e.p[j], sgpr_const(0x1.1111111122322p-7));
        else if constexpr (S == 9)
            e.p[j] = fma(e.r[j], e.p[j], sgpr_const(0x1.55555555502a1p-5));
        else if constexpr (S == 10)
            e.p[j] = fma(e.r[j], e.p[j], sgpr_const(0x1.5555555555511p-3));
        else if constexpr (S == 11)
            e.p[j] = fma(e.r[j], e.p[j], sgpr_const(0x1.000000000000bp-1));
        else if constexpr (S == 12)
            e.p[j] = fma(e.r[j], e.p[j], 1.0);
        else if constexpr (S == 13)
            e.p[j] = fma(e.r[j], e.p[j], 1.0);
        else if constexpr (S == 14) {
            double v = ldexp(e.p[j], (int)e.n[j]);
            v = e.x[j] > 1024.0 ? __builtin_huge_val() : v;
            e.p[j] = e.x[j] < -1075.0 ? 0.0 : v;            // the result
        }
    }
}
template <int B, int E>
__device__ __forceinline__ void exp4_slices(Exp4 &e)
{
    if constexpr (B < E) {
        exp4_slice<B>(e);
        exp4_slices<B + 1, E>(e);
    }
}

template <int MT, int WPS, int TB>
__global__ __launch_bounds__(TB, WPS) void k_transit_mfma_rows(
    double *spectrum, const double *ec, const double *qblk, const double *radius, int nblk,
    double rstar, int itop, int ibottom, double maxdepth, int nlayers, int nwave,
    const int32_t *scatter, TileLimit lim, int32_t *flags)
{
    extern __shared__ __align__(16) double s_q[];         // [nblk][64] | rad[16 MT]
    const int w = blockIdx.y;
    if (lim.gate && uniform_i32(lim.gate + w) == 0)
        return;                                           // (repair pass: walker w was not flagged)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nimpact = min(ibottom, nlayers) - itop;
    double *s_rad = s_q + (size_t)nblk * 64;
    {
        stage_qblocks<MT, TB>(s_q, qblk + (int64_t)w * nblk * 64, tid);
        for (int r = tid; r < 16 * MT; r += TB)
            s_rad[r] = r < nimpact ? radius[(int64_t)w * nlayers + itop + r] : 0.0;
    }
    __syncthreads();
    const int c0 = (blockIdx.x * (TB / 64) + wave) * 32;
    if (c0 >= nwave)
        return;                                           // (after the only barrier)
    const int kq = lane >> 4, n = lane & 15;
    const int col0 = c0 + 2 * n;
    const bool ok[2] = {col0 < nwave, col0 + 1 < nwave};
    const int cpair = max(min(col0, nwave - 2), 0);
    const bool second = col0 != cpair;
    const double *src = ec + ((int64_t)w * nlayers + itop) * nwave + cpair;
    const int KS = (nimpact + 3) / 4;
    double b[4 * MT][2];
    auto loadb = [&](auto mbc) {
        constexpr int mb = decltype(mbc)::value;
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            const int j = min(4 * (4 * mb + kk) + kq, nimpact - 1);
            const d2u v = *reinterpret_cast<const d2u *>(src + (int64_t)j * nwave);
            b[4 * mb + kk][0] = second ? v.y : v.x;
            b[4 * mb + kk][1] = v.y;
        }
    };
    const double rtop = s_rad[0];
    const double *srad = s_rad + kq;
    const int src_lane = (lane + 48) & 63;                // the lane one row above (16 below)
    int first[2] = {ok[0] ? INT_MAX : -1, ok[1] ? INT_MAX : -1};   // (-1: nothing to wait for)
    double acc[2] = {0.0, 0.0}, carry[2] = {0.0, 0.0};
    const double *sq = s_q + lane;
    bool done = false;
    // the last row tile whose layers were interpolated for these 32 columns (TileLimit)
    const int mlim = lim.tile ? uniform_i32(lim.tile + (c0 >> 8)) : MT;
    bool overrun = false;
    loadb(std::integral_constant<int, 0>{});
    auto tile = [&](auto mc) {
        constexpr int m = decltype(mc)::value;
        if (done || 4 * m >= KS)                          // uniform
            return;
        if (m > mlim) {                                   // uniform: a column is still open beyond
            overrun = true;                               // what was interpolated -> repair pass
            done = true;
            return;
        }
        // the next tile's layers are requested before this tile's products (two tiles ahead:
        // measured slower, 1.27 against 1.16 ms at C5's shape -- the loads an exit wastes)
        // (not beyond the tile limit: those layers were never interpolated and an open column
        // there goes to the repair pass -- a fifth of the kernel's reads at C5's shape)
        if constexpr (m + 1 < MT)                         // (clamped rows: harmless past the end)
            if (m + 1 <= mlim || lim.row0 < 0)            // uniform (row0 < 0: A/B switch)
                loadb(std::integral_constant<int, m + 1>{});
        // Column tile 0's products; then column tile 1's with the exponentials of tile 0's rows
        // between them: a product holds the matrix pipe for 64 cycles, the slices issue meanwhile
        // (pinned by scheduling barriers: left alone, the compiler keeps the products together).
        // Tile 0's exponentials are computed for all four rows and selected afterwards.  Same bits;
        // 1.19 against 1.21 ms per 64 walkers at C5's shape.
        v4d C[2] = {v4d{0.0, 0.0, 0.0, 0.0}, v4d{0.0, 0.0, 0.0, 0.0}};
        Exp4 e0;
        {
            constexpr int K = 4 * m + 4;
#pragma unroll
            for (int ks = 0; ks < K; ks++)
                C[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(sq[(qblocks(m) + ks) * 64], b[ks][0], C[0],
                                                            0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; j++)
                e0.x[j] = -C[0][j];
            __builtin_amdgcn_sched_barrier(0);
            static_for_rows<0, K>([&](auto ksc) {
                constexpr int ks = decltype(ksc)::value;
                C[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(sq[(qblocks(m) + ks) * 64], b[ks][1], C[1],
                                                            0, 0, 0);
                exp4_slices<(ks * kExp4Slices) / K, ((ks + 1) * kExp4Slices) / K>(e0);
                __builtin_amdgcn_sched_barrier(0);
            });
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {
            int f = INT_MAX;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int r = 16 * m + 4 * j + kq;
                if (r < nimpact && C[t][j] > maxdepth)
                    f = min(f, r);
            }
            f = min(f, __shfl_xor(f, 16));
            f = min(f, __shfl_xor(f, 32));
            // (an earlier tile's crossing is below every row of this one)
            const int fst = first[t] == INT_MAX ? f : first[t];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int r = 16 * m + 4 * j + kq;
                const bool in = r < nimpact && r <= fst;
                const double rr = srad[16 * m + 4 * j];
                double fv;
                if (t == 0)
                    fv = in ? e0.p[j] * rr : 0.0;
                else
                    fv = in ? pb::exp_s(-C[t][j]) * rr : 0.0;
                const double up = __shfl(fv, src_lane);   // q > 0: row r - 1; q = 0: row r + 3
                const double fprev = kq > 0 ? up : carry[t];
                carry[t] = up;
                if (in && r >= 1)
                    acc[t] += (rr - srad[16 * m + 4 * j - 1]) * (fprev + fv);
            }
            first[t] = fst;
        }
        done = __all(first[0] != INT_MAX && first[1] != INT_MAX);
    };
    static_assert(MT <= 8, "row tiles");
    tile(std::integral_constant<int, 0>{});
    if constexpr (MT > 1) tile(std::integral_constant<int, 1>{});
    if constexpr (MT > 2) tile(std::integral_constant<int, 2>{});
    if constexpr (MT > 3) tile(std::integral_constant<int, 3>{});
    if constexpr (MT > 4) tile(std::integral_constant<int, 4>{});
    if constexpr (MT > 5) tile(std::integral_constant<int, 5>{});
    if constexpr (MT > 6) tile(std::integral_constant<int, 6>{});
    if constexpr (MT > 7) tile(std::integral_constant<int, 7>{});
    if (overrun) {
        if (lane == 0 && flags) {
            flags[w] = 1;
            flags[gridDim.y] = 1;                         // flags[nwalkers]: any walker
        }
        return;                                           // (the repair pass writes these columns)
    }
#pragma unroll
    for (int t = 0; t < 2; t++) {
        double a = acc[t];
        a += __shfl_xor(a, 16);
        a += __shfl_xor(a, 32);
        if (kq == 0 && ok[t]) {
            const int64_t dst = scatter ? scatter[col0 + t] : col0 + t;
            // (an index outside the grid -- a caller's column_d that is not a permutation -- is
            // dropped, not written out of bounds)
            if (dst >= 0 && dst < nwave)
                spectrum[(int64_t)w * nwave + dst] =
                    (rtop * rtop + 2 * (a * 0.5)) / (rstar * rstar);
        }
    }
}

#ifdef PB_EXPERIMENTS   // LDS column tile of the fused transit kernel (5x slower; A/B only)
// ---------------------------------------------------------------------------
// The same pass with the column tile in LDS: workgroup = 64 columns x NB wavefronts, wavefront b
// owning the impact parameters 16b .. 16b+15.  The tile of s_i = ec[i+1] + ec[i] (64 columns x all
// segments) is read from HBM ONCE, cooperatively and coalesced, and every wavefront then takes
// its operands from LDS (the one-thread-per-column form above re-reads the column once per row
// block: 3x the bytes at 80 layers, all from HBM once the batch outgrows the caches).  The early
// exit and the transmission integral then run down the rows wavefront after wavefront, the
// carried state (first crossing, trapezoid sum, previous integrand) passing through LDS.
// ---------------------------------------------------------------------------
constexpr int kTileRows = 16;

__global__ __launch_bounds__(1024) void k_transit_tile(
    double *depth, int32_t *ideep, double *spectrum, const double *ec, const double *raypath,
    const double *radius, int64_t npath, double rstar, int itop, int ibottom, double maxdepth,
    int nlayers, int nwave, int deck_row, double rsurf)
{
    extern __shared__ __align__(16) double s_mem[];
    const int w = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nwaves = blockDim.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const bool active = col < nwave;
    const int64_t plane = (int64_t)nlayers * nwave;
    ec += (int64_t)w * plane;
    if (depth)
        depth += (int64_t)w * plane;
    const double *path = raypath ? raypath + (int64_t)w * npath : nullptr;
    const double *rad = radius ? radius + (int64_t)w * nlayers : nullptr;
    const int nimpact = min(ibottom, nlayers) - itop;     // rows 0..nimpact-1 are evaluated
    const int nseg_all = max(nimpact - 1, 0);
    double *s_tile = s_mem;                               // [segment][64]
    double *s_carry = s_tile + (size_t)nseg_all * 64;     // [3][64]: acc, fprev, rprev
    int *s_stop = reinterpret_cast<int *>(s_carry + 3 * 64);   // [64]
    double *s_path = reinterpret_cast<double *>(s_stop + 64);  // per wavefront [segment][16]

    // the tile: row i of s = ec[itop+i+1] + ec[itop+i]; wavefront v loads rows v, v+nwaves, ...
    // (each row 512 contiguous bytes); the two operands of a row are two coalesced loads
    {
        const double *src = ec + (int64_t)itop * nwave + (active ? col : 0);
        for (int i = wave; i < nseg_all; i += nwaves) {
            const double a = src[(int64_t)i * nwave], b = src[(int64_t)(i + 1) * nwave];
            s_tile[i * 64 + lane] = b + a;
        }
    }
    // my block of rows and its ray paths ([segment][row], zero where segment >= row)
    const int rb = wave * kTileRows;
    const int rlast = min(rb + kTileRows, nimpact) - 1;
    const int nseg = rb <= rlast ? max(rlast, 0) : 0;
    int poff = 0;                                         // doubles before my block
    for (int v = 0; v < wave; v++)
        poff += max(min(v * kTileRows + kTileRows, nimpact) - 1, 0) * kTileRows;
    double *mypath = s_path + poff;
    for (int e = lane; e < nseg * kTileRows; e += 64) {
        const int i = e / kTileRows, k = e % kTileRows;
        const int r = rb + k;
        mypath[e] = (r <= rlast && i < r) ? path[((int64_t)r * (r - 1)) / 2 + i] : 0.0;
    }
    if (threadIdx.x < 64) {
        s_stop[lane] = -1;
        s_carry[lane] = 0.0;
        s_carry[64 + lane] = 0.0;
        s_carry[128 + lane] = 0.0;
    }
    __syncthreads();
    double tau[kTileRows];
#pragma unroll
    for (int k = 0; k < kTileRows; k++)
        tau[k] = 0.0;
    for (int i = 0; i < nseg; i++) {
        const double s = s_tile[i * 64 + lane];
        const double *pk = mypath + i * kTileRows;              // LDS broadcast reads
#pragma unroll
        for (int k = 0; k < kTileRows; k++)
            tau[k] += pk[k] * s;
    }
    if (depth && active && wave == 0)
        for (int r = 0; r < itop; r++)
            depth[(int64_t)r * nwave + col] = 0.0;
    // the rows in order, one wavefront after the other
    for (int v = 0; v < nwaves; v++) {
        if (v == wave && rb <= rlast) {
            int stop = s_stop[lane];
            double acc = s_carry[lane], fprev = s_carry[64 + lane], rprev = s_carry[128 + lane];
#pragma unroll
            for (int k = 0; k < kTileRows; k++) {
                const int r = rb + k;
                if (r > rlast)
                    break;
                double t = tau[k];
                if (stop < 0) {
                    if (spectrum) {
                        const double rr = rad[itop + r];
                        double f = pb::exp_s(-t) * rr;
                        if (r > 0 && r == deck_row) {
                            f = deck_integrand(fprev, f, rprev, rr, rsurf);
                            acc += (rsurf - rprev) * (fprev + f);
                        } else if (r > 0) {
                            acc += (rr - rprev) * (fprev + f);
                        }
                        fprev = f;
                        rprev = rr;
                    }
                    if (t > maxdepth)
                        stop = r;
                } else {
                    t = 0.0;
                }
                if (depth && active)
                    depth[(int64_t)(itop + r) * nwave + col] = t;
            }
            s_stop[lane] = stop;
            s_carry[lane] = acc;
            s_carry[64 + lane] = fprev;
            s_carry[128 + lane] = rprev;
        }
        __syncthreads();
    }
    if (!active)
        return;
    if (depth)
        for (int r = max(nimpact, 0) + wave; r < nlayers - itop; r += nwaves)
            depth[(int64_t)(itop + r) * nwave + col] = 0.0;   // rows at and below ibottom
    if (wave == 0) {
        const int stop = s_stop[lane];
        const int last = nimpact > 0 ? itop + nimpact - 1 : itop;
        if (ideep)
            ideep[(int64_t)w * nwave + col] = stop >= 0 ? itop + stop : last;
        if (spectrum) {
            const double rtop = rad[itop];
            spectrum[(int64_t)w * nwave + col] =
                (rtop * rtop + 2 * (s_carry[lane] * 0.5)) / (rstar * rstar);
        }
    }
}

#endif  // PB_EXPERIMENTS

// ---------------------------------------------------------------------------
// one transit launch: environment, plan, ray-path layout, then the kernel of the planned form
// ---------------------------------------------------------------------------

// The PB_* variables a launch consults.  Read once at the top of EVERY launch, never kept in a
// static: the tests change them between calls of one process.
struct TransitTuning {
    int mfma = -1;                 // PB_TRANSIT_MFMA: 0 = vector kernels, 4 = layers-outer (experiments); -1 = not set
    int rows = 0;                  // PB_TRANSIT_ROWS as 8 or 16 (any value >= 16); 0 = not set
    bool no_scalar = false;        // PB_TRANSIT_SCALAR=0: ray paths staged in LDS
    bool prefetch_all = false;     // PB_C5_PREFETCH_ALL=1: the next tile's layers are requested whatever the limit -- A/B
    bool tile = false;             // PB_TRANSIT_TILE=1 (experiments build): the LDS-tile form
};

static TransitTuning read_transit_tuning()
{
    TransitTuning t;
    if (const char *e = getenv("PB_TRANSIT_MFMA"))
        t.mfma = atoi(e);
    if (const char *e = getenv("PB_TRANSIT_ROWS"))
        t.rows = atoi(e) >= 16 ? 16 : 8;
    if (const char *e = getenv("PB_TRANSIT_SCALAR"))
        t.no_scalar = atoi(e) == 0;
    if (const char *e = getenv("PB_C5_PREFETCH_ALL"))
        t.prefetch_all = atoi(e) != 0;
#ifdef PB_EXPERIMENTS
    if (const char *e = getenv("PB_TRANSIT_TILE"))
        t.tile = atoi(e) != 0;
#endif
    return t;
}

// What a launch will run, decided from the call and the environment alone.
enum class TransitForm {
    MfmaRows,      // k_transit_mfma_rows: the retrieval batch on the matrix cores
    Pair,          // k_transit_pair: two columns per thread, ray paths in SGPRs
    ScalarPath,    // k_transit_fused<rows, true>: one column per thread, ray paths in SGPRs
    Lds,           // k_transit_fused<rows, false>: one column per thread, ray paths staged in LDS
#ifdef PB_EXPERIMENTS
    MfmaLayers,    // k_transit_mfma: the layers-outer matrix kernel (PB_TRANSIT_MFMA=4)
    Tile,          // k_transit_tile: the column tile in LDS (PB_TRANSIT_TILE=1)
#endif
};

struct TransitPlan {
    TransitForm form = TransitForm::Lds;
    int rows = 0;                    // impact parameters per block (Pair, ScalarPath, Lds)
    int mt = 0;                      // row tiles (matrix cores); their launch step names the (W, T)
    // the layout of call.work, per walker: the path blocks of k_path_blocks (plen doubles) or the Q
    // blocks of k_path_qblocks (qblocks(mt) x 64 doubles); whether this launch builds it
    bool build_path_blocks = false, build_qblocks = false;
    int64_t plen = 0;                // ray-path doubles per walker as the kernel reads them
    TileLimit lim{nullptr, 0, nullptr};
    size_t lds = 0;                  // dynamic LDS bytes
    dim3 grid;                       // (matrix cores: set by the launch step from its T)
    int block = kBlock;
};

// rows per block of the fused kernel for a launch of nwave x nwalkers columns
static int fused_rows(int nwave, int nwalkers, int nrow, const TransitTuning &tn)
{
    // measured at C5's shape (64 walkers x 1e5 columns x 80 layers, ray paths in SGPRs): 8 rows
    // per thread 3.97 ms, 16 rows 3.55 ms, 40 rows 3.70 ms (157 registers; since removed); LDS-staged paths 4.68
    int rows = (int64_t)nwave * nwalkers <= 32768 ? 8 : 16;
    if (tn.rows)
        rows = tn.rows;
    if (rows > 8 && (size_t)std::max(nrow, 1) * rows * 8 > 64 * 1024)
        rows = 8;
    return rows;
}

static int64_t blocked_len(int rows, int nimpact)
{
    int64_t n = 0;
    for (int rb = 0; rb < nimpact; rb += rows)
        n += (int64_t)std::max(std::min(rb + rows, nimpact) - 1, 0) * rows;
    return n;
}

// can the call run on the matrix cores?  (spectrum only, no deck, 2 ... 128 impact parameters)
static bool mfma_shape(const TransitCall &c, int nimpact, int mt)
{
    return c.work && c.spectrum && !c.depth && !c.ideep && c.deck_row < 0 && nimpact > 1 &&
           mt <= 8 && c.nwave >= 2;
}

static TransitPlan plan_transit(const TransitCall &c, const TransitTuning &tn)
{
    TransitPlan p;
    const int nrow = c.nlayers - c.itop;
    const int nimpact = std::min(c.ibottom, c.nlayers) - c.itop;
    p.lim = TileLimit{c.tile_limit, tn.prefetch_all ? -1 : c.itop, c.gate};
#ifdef PB_EXPERIMENTS
    // PB_TRANSIT_TILE=1: the LDS-tile form (measured slower: 10.3 ms against 4.5 ms per 64-walker
    // batch at C5's shape -- five wavefronts of uneven length per 70 KB of LDS); kept for A/B
    if (tn.tile) {
        const int nb = std::max(1, pb::div_up(std::max(nimpact, 1), kTileRows));
        size_t npd = 0;
        for (int v = 0; v < nb; v++)
            npd += (size_t)std::max(std::min(v * kTileRows + kTileRows, nimpact) - 1, 0) * kTileRows;
        const size_t tl = ((size_t)std::max(nimpact - 1, 0) * 64 + 3 * 64 + npd) * 8 + 64 * 4;
        if (nb <= 16 && tl <= 150 * 1024) {
            p.form = TransitForm::Tile;
            p.plen = c.npath;
            p.lds = tl;
            p.grid = dim3(pb::div_up(c.nwave, 64), c.nwalkers);
            p.block = nb * 64;
            return p;
        }
    }
#endif  // PB_EXPERIMENTS
    // the retrieval batch (spectrum only, no deck) on the matrix cores: k_transit_mfma_rows
    const bool no_mfma = tn.mfma == 0 && !c.scatter;              // (ordered: this form only)
    const int mt = pb::div_up(std::max(nimpact, 1), 16);
    if (!no_mfma && mfma_shape(c, nimpact, mt) && c.nwalkers >= 1) {
        // row tile by row tile with the early exit (the default: 1.48 against 1.59 ms per 64
        // walkers at C5's shape with the columns in grid order, 1.16 with ordered columns);
        // PB_TRANSIT_MFMA=4 (experiments build): the layers-outer kernel it replaced, for A/B
        p.form = TransitForm::MfmaRows;
#ifdef PB_EXPERIMENTS
        if (!c.scatter && tn.mfma == 4)
            p.form = TransitForm::MfmaLayers;
#endif
        p.mt = mt;
        p.build_qblocks = !c.gate;   // (a gated repair pass re-uses the Q blocks of its first pass)
        p.lds = ((size_t)qblocks(mt) * 64 + (size_t)mt * 16) * 8;
        return p;
    }
    const bool scalar = c.work != nullptr && nimpact > 1 && !tn.no_scalar;
    p.rows = fused_rows(c.nwave, c.nwalkers, nrow, tn);
    p.grid = dim3(pb::div_up(c.nwave, kBlock), c.nwalkers);
    p.plen = c.npath;
    if (!scalar) {
        p.form = TransitForm::Lds;
        p.lds = (size_t)std::max(nrow, 1) * p.rows * 8;
        return p;
    }
    p.form = TransitForm::ScalarPath;
    p.build_path_blocks = true;
    p.plen = blocked_len(p.rows, nimpact);
    if (p.rows == 16 && !c.depth && !c.ideep && c.nwalkers > 1 && c.deck_row < 0 && c.spectrum) {
        // the retrieval batch, two columns per thread
        p.form = TransitForm::Pair;
        p.grid = dim3(pb::div_up(c.nwave, 2 * kBlock), c.nwalkers);
    }
    return p;
}

// a kernel whose dynamic LDS exceeds the 64 KiB every kernel may use
static int allow_lds(const void *kern, size_t lds)
{
    if (lds > 64 * 1024)
        PB_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return PB_OK;
}

template <int M, int W, int T>
static int run_mfma_rows(const TransitCall &c, const TransitPlan &p, hipStream_t s)
{
    const int rc = allow_lds(reinterpret_cast<const void *>(k_transit_mfma_rows<M, W, T>), p.lds);
    if (rc != PB_OK)
        return rc;
    // threads per workgroup: a workgroup stages its walker's Q blocks (30 KB at 80
    // layers) once for T / 64 x 32 columns
    dim3 grid(pb::div_up(c.nwave, (T / 64) * 32), c.nwalkers);
    k_transit_mfma_rows<M, W, T><<<grid, T, p.lds, s>>>(
        c.spectrum, c.ec, c.work, c.radius, qblocks(M), c.rstar, c.itop, c.ibottom, c.maxdepth,
        c.nlayers, c.nwave, c.scatter, p.lim, c.flags);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

static int launch_mfma_rows(const TransitCall &c, const TransitPlan &p, hipStream_t s)
{
    switch (p.mt) {
    case 1: return run_mfma_rows<1, 4, 256>(c, p, s);
    case 2: return run_mfma_rows<2, 4, 256>(c, p, s);
    case 3: return run_mfma_rows<3, 4, 256>(c, p, s);
    case 4: return run_mfma_rows<4, 4, 256>(c, p, s);
    // 80 layers: the B operands alone are 80 registers.  Three wavefronts per SIMD
    // of up to 168 registers (no spills) beat four of 128 (24 spilled): 1.23
    // against 1.31 ms per 64 walkers at C5's shape
    case 5: return run_mfma_rows<5, 3, 256>(c, p, s);
    case 6: return run_mfma_rows<6, 2, 256>(c, p, s);
    case 7: return run_mfma_rows<7, 2, 256>(c, p, s);
    default: return run_mfma_rows<8, 2, 256>(c, p, s);
    }
}

static int launch_pair(const TransitCall &c, const TransitPlan &p, hipStream_t s)
{
    k_transit_pair<16><<<p.grid, kBlock, 0, s>>>(c.spectrum, c.ec, c.work, c.radius, p.plen, c.rstar,
                                                c.itop, c.ibottom, c.maxdepth, c.nlayers, c.nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

// one column per thread: ray paths from call.work in SGPRs (kScalarPath), else staged in LDS
template <int R, bool kScalarPath>
static int run_fused(const TransitCall &c, const TransitPlan &p, hipStream_t s)
{
    k_transit_fused<R, kScalarPath><<<p.grid, kBlock, p.lds, s>>>(
        c.depth, c.ideep, c.spectrum, c.ec, kScalarPath ? c.work : c.raypath, c.radius, p.plen,
        c.rstar, c.itop, c.ibottom, c.maxdepth, c.nlayers, c.nwave, c.deck_row, c.rsurf);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

static int launch_scalar_path(const TransitCall &c, const TransitPlan &p, hipStream_t s)
{
    return p.rows == 16 ? run_fused<16, true>(c, p, s) : run_fused<8, true>(c, p, s);
}

static int launch_lds(const TransitCall &c, const TransitPlan &p, hipStream_t s)
{
    return p.rows == 16 ? run_fused<16, false>(c, p, s) : run_fused<8, false>(c, p, s);
}

#ifdef PB_EXPERIMENTS
template <int M, int W, int T>
static int run_mfma_layers(const TransitCall &c, const TransitPlan &p, hipStream_t s)
{
    const int rc = allow_lds(reinterpret_cast<const void *>(k_transit_mfma<M, W, T>), p.lds);
    if (rc != PB_OK)
        return rc;
    dim3 grid(pb::div_up(c.nwave, (T / 64) * 32), c.nwalkers);
    k_transit_mfma<M, W, T><<<grid, T, p.lds, s>>>(c.spectrum, c.ec, c.work, c.radius, qblocks(M),
                                                    c.rstar, c.itop, c.ibottom, c.maxdepth,
                                                    c.nlayers, c.nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

static int launch_mfma_layers(const TransitCall &c, const TransitPlan &p, hipStream_t s)
{
    switch (p.mt) {
    case 1: return run_mfma_layers<1, 4, 256>(c, p, s);
    case 2: return run_mfma_layers<2, 4, 256>(c, p, s);
    case 3: return run_mfma_layers<3, 4, 256>(c, p, s);
    case 4: return run_mfma_layers<4, 4, 256>(c, p, s);
    case 5: return run_mfma_layers<5, 4, 512>(c, p, s);
    case 6: return run_mfma_layers<6, 2, 256>(c, p, s);
    case 7: return run_mfma_layers<7, 2, 256>(c, p, s);
    default: return run_mfma_layers<8, 2, 256>(c, p, s);
    }
}

static int launch_tile(const TransitCall &c, const TransitPlan &p, hipStream_t s)
{
    const int rc = allow_lds(reinterpret_cast<const void *>(k_transit_tile), p.lds);
    if (rc != PB_OK)
        return rc;
    k_transit_tile<<<p.grid, p.block, p.lds, s>>>(c.depth, c.ideep, c.spectrum, c.ec, c.raypath,
                                                 c.radius, c.npath, c.rstar, c.itop, c.ibottom,
                                                 c.maxdepth, c.nlayers, c.nwave, c.deck_row,
                                                 c.rsurf);
    PB_LAUNCH_CHECK();
    return PB_OK;
}
#endif  // PB_EXPERIMENTS

}  // namespace

namespace pbt {

int launch_path_qblocks(double *qblk_d, const double *raypath_d, int64_t npath, int mt, int nimpact,
                        int nwalkers, hipStream_t s)
{
    const int nblk = qblocks(mt);
    dim3 qgrid((unsigned)std::min(16, pb::div_up((int64_t)nblk * 64, kBlock)), nwalkers);
    k_path_qblocks<<<qgrid, kBlock, 0, s>>>(qblk_d, raypath_d, npath, nblk, nimpact);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace pbt

int pb_transit_fused_launch(const TransitCall &c, hipStream_t s)
{
    const int nimpact = std::min(c.ibottom, c.nlayers) - c.itop;
    PB_REQUIRE(!c.scatter || mfma_shape(c, nimpact, pb::div_up(std::max(nimpact, 1), 16)),
               "pb_transit_spectrum_ordered: 2 ... 128 impact parameters and at least 2 "
               "columns (got %d, %d)", nimpact, c.nwave);
    const TransitPlan p = plan_transit(c, read_transit_tuning());
    if (p.build_qblocks) {
        const int rc = pbt::launch_path_qblocks(c.work, c.raypath, c.npath, p.mt, nimpact,
                                                c.nwalkers, s);
        if (rc != PB_OK)
            return rc;
    }
    if (p.build_path_blocks) {
        dim3 bgrid((unsigned)std::min<int64_t>(64, pb::div_up(p.plen, kBlock)), c.nwalkers);
        k_path_blocks<<<bgrid, kBlock, 0, s>>>(c.work, c.raypath, c.npath, p.plen, p.rows, nimpact);
        PB_LAUNCH_CHECK();
    }
    switch (p.form) {
    case TransitForm::MfmaRows: return launch_mfma_rows(c, p, s);
    case TransitForm::Pair: return launch_pair(c, p, s);
    case TransitForm::ScalarPath: return launch_scalar_path(c, p, s);
    case TransitForm::Lds: return launch_lds(c, p, s);
#ifdef PB_EXPERIMENTS
    case TransitForm::MfmaLayers: return launch_mfma_layers(c, p, s);
    case TransitForm::Tile: return launch_tile(c, p, s);
#endif
    }
    return PB_OK;
}

// the blocked ray-path layout for one spectrum in the stream's persistent scratch (pb_core.hip);
// PB_ERR_NOMEM when there is none: the caller falls back to the LDS form
int pb_path_blocks_launch(double **blocked_d, int64_t *len, const double *raypath_d, int64_t npath,
                          int rows, int nimpact, hipStream_t s)
{
    const int64_t plen = blocked_len(rows, nimpact);
    *blocked_d = nullptr;
    *len = plen;
    if (plen <= 0)
        return PB_ERR_ARG;
    double *buf = reinterpret_cast<double *>(pb::stream_scratch(s, (size_t)plen * 8));
    if (!buf)
        return PB_ERR_NOMEM;
    dim3 bgrid((unsigned)std::min<int64_t>(64, pb::div_up(plen, kBlock)), 1);
    k_path_blocks<<<bgrid, kBlock, 0, s>>>(buf, raypath_d, npath, plen, rows, nimpact);
    if (hipGetLastError() != hipSuccess)
        return PB_ERR_HIP;
    *blocked_d = buf;
    return PB_OK;
}

extern "C" {

int pb_transit_path(double *raypath_d, const double *radius_d, int itop, int nlayers,
                    int nwalkers, void *stream)
{
    PB_REQUIRE(nlayers >= 1 && itop >= 0 && itop < nlayers && nwalkers >= 0,
               "pb_transit_path: bad shape");
    const int nrow = nlayers - itop;
    if (nwalkers == 0 || nrow < 2)
        return PB_OK;
    PB_REQUIRE(raypath_d && radius_d, "pb_transit_path: null pointer");
    const int64_t npath = ((int64_t)nrow * (nrow - 1)) / 2;
    dim3 grid(std::min(nrow, 64), nwalkers);
    k_transit_path<<<grid, kBlock, 0, pb::as_stream(stream)>>>(raypath_d, radius_d, itop, nlayers,
                                                             npath);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int64_t pb_transit_work_doubles(int nlayers, int itop, int ibottom, int nwave, int nwalkers)
{
    if (nlayers < 1 || itop < 0 || itop >= nlayers)
        return 0;
    const int nimpact = std::min(ibottom, nlayers) - itop;
    // the largest layout any row-block choice needs
    int64_t n = 0;
    for (int rows : {8, 16})
        n = std::max(n, blocked_len(rows, nimpact));
    // ... and the 16 x 4 blocks of the matrix-core form (k_path_qblocks)
    n = std::max<int64_t>(n, (int64_t)qblocks(pb::div_up(std::max(nimpact, 1), 16)) * 64);
    (void)nwave;
    return n * std::max(nwalkers, 0) + 8;
}

int pb_transit_spectrum_batch(double *spectrum_d, double *depth_d, int32_t *ideep_d,
                              const double *ec_d, const double *raypath_d,
                              const double *radius_d, double rstar, int itop, int ibottom,
                              double maxdepth, int nlayers, int nwave, int nwalkers,
                              void *work_d, void *stream)
{
    PB_REQUIRE(nlayers > 0 && nwave >= 0 && nwalkers >= 0, "pb_transit_spectrum_batch: bad shape");
    PB_REQUIRE(itop >= 0 && itop < nlayers, "pb_transit_spectrum_batch: itop out of range");
    PB_REQUIRE(ibottom <= nlayers, "pb_transit_spectrum_batch: ibottom > nlayers");
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    const int nrow = nlayers - itop;
    PB_REQUIRE(spectrum_d && ec_d && radius_d && (nrow == 1 || raypath_d),
               "pb_transit_spectrum_batch: null pointer");
    TransitCall c;
    c.depth = depth_d;
    c.ideep = ideep_d;
    c.spectrum = spectrum_d;
    c.ec = ec_d;
    c.raypath = raypath_d;
    c.radius = radius_d;
    c.npath = ((int64_t)nrow * (nrow - 1)) / 2;
    c.rstar = rstar;
    c.itop = itop;
    c.ibottom = ibottom;
    c.maxdepth = maxdepth;
    c.nlayers = nlayers;
    c.nwave = nwave;
    c.nwalkers = nwalkers;
    c.work = reinterpret_cast<double *>(work_d);
    return pb_transit_fused_launch(c, pb::as_stream(stream));
}

int pb_transit_spectrum_ordered(double *spectrum_d, const double *ec_d, const double *raypath_d,
                                const double *radius_d, const int32_t *column_d, double rstar,
                                int itop, int ibottom, double maxdepth, int nlayers, int nwave,
                                int nwalkers, void *work_d, void *stream)
{
    PB_REQUIRE(nlayers > 0 && nwave >= 0 && nwalkers >= 0, "pb_transit_spectrum_ordered: bad shape");
    PB_REQUIRE(itop >= 0 && itop < nlayers, "pb_transit_spectrum_ordered: itop out of range");
    PB_REQUIRE(ibottom <= nlayers, "pb_transit_spectrum_ordered: ibottom > nlayers");
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    const int nrow = nlayers - itop;
    PB_REQUIRE(spectrum_d && ec_d && radius_d && raypath_d && column_d && work_d,
               "pb_transit_spectrum_ordered: null pointer");
    TransitCall c;
    c.spectrum = spectrum_d;
    c.ec = ec_d;
    c.raypath = raypath_d;
    c.radius = radius_d;
    c.npath = ((int64_t)nrow * (nrow - 1)) / 2;
    c.rstar = rstar;
    c.itop = itop;
    c.ibottom = ibottom;
    c.maxdepth = maxdepth;
    c.nlayers = nlayers;
    c.nwave = nwave;
    c.nwalkers = nwalkers;
    c.work = reinterpret_cast<double *>(work_d);
    c.scatter = column_d;
    return pb_transit_fused_launch(c, pb::as_stream(stream));
}

int pb_transit_spectrum_limited(double *spectrum_d, const double *ec_d, const double *raypath_d,
                                const double *radius_d, const int32_t *column_d, double rstar,
                                int itop, int ibottom, double maxdepth, int nlayers, int nwave,
                                int nwalkers, void *work_d, const int32_t *tile_limit_d,
                                int32_t *flags_d, const int32_t *gate_d, void *stream)
{
    PB_REQUIRE(nlayers > 0 && nwave >= 0 && nwalkers >= 0, "pb_transit_spectrum_limited: bad shape");
    PB_REQUIRE(itop >= 0 && itop < nlayers, "pb_transit_spectrum_limited: itop out of range");
    PB_REQUIRE(ibottom <= nlayers, "pb_transit_spectrum_limited: ibottom > nlayers");
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    const int nrow = nlayers - itop;
    PB_REQUIRE(spectrum_d && ec_d && radius_d && raypath_d && column_d && work_d,
               "pb_transit_spectrum_limited: null pointer");
    PB_REQUIRE(!tile_limit_d || flags_d,
               "pb_transit_spectrum_limited: a tile limit needs flags[nwalkers + 1] to report the "
               "walkers that ran past it");
    TransitCall c;
    c.spectrum = spectrum_d;
    c.ec = ec_d;
    c.raypath = raypath_d;
    c.radius = radius_d;
    c.npath = ((int64_t)nrow * (nrow - 1)) / 2;
    c.rstar = rstar;
    c.itop = itop;
    c.ibottom = ibottom;
    c.maxdepth = maxdepth;
    c.nlayers = nlayers;
    c.nwave = nwave;
    c.nwalkers = nwalkers;
    c.work = reinterpret_cast<double *>(work_d);
    c.scatter = column_d;
    c.tile_limit = tile_limit_d;
    c.flags = flags_d;
    c.gate = gate_d;
    return pb_transit_fused_launch(c, pb::as_stream(stream));
}

}  // extern "C"
