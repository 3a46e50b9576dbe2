// The fused transit pass, shared by its users: what a launch is asked for (TransitCall), the
// functions that cross files (pb_transit.hip defines them) and the device pieces the matrix-core
// kernels of pb_transit.hip and pb_table_transit.hip have in common.
#pragma once

#include <climits>

#include "pb_common.h"

// One launch of the fused transit pass (ec -> depth, ideep, spectrum) for nwalkers atmospheres.
// Members left at their defaults are absent.
struct TransitCall {
    // outputs: depth[nwalkers][nlayers][nwave] and ideep[nwalkers][nwave] are optional (a retrieval
    // needs neither); spectrum[nwalkers][nwave]
    double *depth = nullptr;
    int32_t *ideep = nullptr;
    double *spectrum = nullptr;
    const double *ec = nullptr;          // [nwalkers][nlayers][nwave]
    const double *raypath = nullptr;     // [nwalkers][npath], the packed lower triangle of pb_transit_path
    const double *radius = nullptr;      // [nwalkers][nlayers]
    int64_t npath = 0;
    double rstar = 0.0;
    int itop = 0, ibottom = 0;
    double maxdepth = 0.0;
    int nlayers = 0, nwave = 0, nwalkers = 1;
    int deck_row = -1;                   // row of an opaque cloud deck below itop, or none
    double rsurf = 0.0;                  // the deck's radius
    // nwalkers * pb_transit_work_doubles() of scratch for the forms that re-lay the ray paths (path
    // blocks in SGPRs, Q blocks of the matrix cores); absent: ray paths staged in LDS
    double *work = nullptr;
    // ordered columns (TableSpectrum.column_order): the grid index of each column; the layers nobody
    // reads (pb::TileLimit): limits per block of 256 columns, the walkers that ran past them, the
    // repair pass's gate
    const int32_t *scatter = nullptr;
    const int32_t *tile_limit = nullptr;
    int32_t *flags = nullptr;
    const int32_t *gate = nullptr;
};

// shared with pb_transit_one.hip: the single-spectrum entries can use the fused kernel too
int pb_transit_fused_launch(const TransitCall &call, hipStream_t s);
// the blocked ray-path layout for one spectrum in the stream's persistent scratch (pb_core.hip);
// PB_ERR_NOMEM when there is none: the caller falls back to the LDS form
int pb_path_blocks_launch(double **blocked_d, int64_t *len, const double *raypath_d, int64_t npath,
                          int rows, int nimpact, hipStream_t s);

namespace pbt {

// 16 x 4 blocks of Q on or below the diagonal of mt row tiles (k_path_qblocks)
__host__ __device__ constexpr int qblocks(int mt) { return 2 * mt * mt + 2 * mt; }

// every walker's Q blocks (qblocks(mt) x 64 doubles each) from its ray paths: k_path_qblocks
int launch_path_qblocks(double *qblk_d, const double *raypath_d, int64_t npath, int mt, int nimpact,
                        int nwalkers, hipStream_t s);

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));

// Epilogue of the matrix-core transit kernels on the accumulator layout: lane (kq = l >> 4,
// n = l & 15) holds the rows 16m + 4j + kq of one column per 16-column tile.  One tile:
template <int MT>
__device__ __forceinline__ void mfma_transit_epilogue_tile(
    const v4d (&C)[MT], const double *s_rad, double *dst, bool ok, int lane, int nimpact,
    double maxdepth, double rstar)
{
    const int kq = lane >> 4;
    const double rtop = s_rad[0];
    const double *srad = s_rad + kq;
    const int src_lane = (lane + 48) & 63;                // the lane one row above (16 below)
    int first = INT_MAX;
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = 16 * m + 4 * j + kq;
            if (r < nimpact && C[m][j] > maxdepth)
                first = min(first, r);
        }
    first = min(first, __shfl_xor(first, 16));
    first = min(first, __shfl_xor(first, 32));
    double acc = 0.0, carry = 0.0;                        // carry: row 16m + 4j - 1 seen from q = 0
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = 16 * m + 4 * j + kq;
            const bool in = r < nimpact && r <= first;
            const double rr = srad[16 * m + 4 * j];
            const double f = in ? pb::exp_s(-C[m][j]) * rr : 0.0;
            const double up = __shfl(f, src_lane);        // q > 0: row r - 1; q = 0: row r + 3
            const double fprev = kq > 0 ? up : carry;
            carry = up;
            if (in && r >= 1)
                acc += (rr - srad[16 * m + 4 * j - 1]) * (fprev + f);
        }
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    if (kq == 0 && ok)
        *dst = (rtop * rtop + 2 * (acc * 0.5)) / (rstar * rstar);
}

// the two column tiles of a wavefront (columns col0 and col0 + 1 of one walker)
template <int MT>
__device__ __forceinline__ void mfma_transit_epilogue(
    const v4d (&C)[2][MT], const double *s_rad, double *spectrum_w, int col0, const bool (&ok)[2],
    int lane, int nimpact, double maxdepth, double rstar)
{
#pragma unroll
    for (int t = 0; t < 2; t++)
        mfma_transit_epilogue_tile<MT>(C[t], s_rad, spectrum_w + col0 + t, ok[t], lane, nimpact,
                                       maxdepth, rstar);
}

// A walker's Q blocks (qblocks(MT) x 64 doubles: 30 KB at 80 layers) -> LDS.  The count is a
// compile-time constant of the instantiation, so every thread issues ALL of its 16-byte loads
// before the first LDS store: one L2 round trip per workgroup instead of one per 8-byte element of
// a run-time loop (7.5 at 512 threads).
template <int MT, int TB>
__device__ __forceinline__ void stage_qblocks(double *s_q, const double *q, int tid)
{
    constexpr int N2 = qblocks(MT) * 32;                  // 16-byte units
    constexpr int PER = (N2 + TB - 1) / TB;
    const d2u *src = reinterpret_cast<const d2u *>(q);
    d2u tmp[PER];
#pragma unroll
    for (int i = 0; i < PER; i++)
        if (tid + i * TB < N2)
            tmp[i] = src[tid + i * TB];
#pragma unroll
    for (int i = 0; i < PER; i++)
        if (tid + i * TB < N2) {
            s_q[2 * (tid + i * TB)] = tmp[i].x;
            s_q[2 * (tid + i * TB) + 1] = tmp[i].y;
        }
}

}  // namespace pbt
