// Two-stream emission for a batch of walkers (the retrieval inner loop in the geometry of
// rt_path emission_two_stream / eclipse_two_stream): per (walker, column) the chain the
// single-spectrum kernels run as three launches -- k_plane_depth with maxdepth = inf
// (_trapezoid.c:175-213, opacity/optic_depth.py:124-126), k_two_stream_trans, k_two_stream
// (pyrat/spectrum.py:454-522) -- in ONE pass that keeps the running depth, the downward flux and
// the Planck values in registers and stores only flux_up[0].  Same operations in the same order
// (pb_two_stream.h holds the shared statements): the same bits.
//
// What the upward sweep needs again in reverse order, dtau0[i] and trans[i], is STORED by the
// downward sweep rather than recomputed: dtau0[i] over row i of ec (dead once row i + 1 has been
// read; every thread owns its column) and trans[i] in work[nw][L-1][W].  That is 40 B of traffic
// per (interval, column) -- 8 read + 16 written going down, 16 read going up -- against a second
// exp1 (a 25-term series or a continued fraction of 20 + 80/x FP64 divisions) per cell if trans
// were recomputed.  exp(-dtau0) is recomputed on the way up (25 instructions, no traffic).
#include "pb_common.h"
#include "pb_planck.h"
#include "pb_two_stream.h"

namespace {

constexpr int kBlock = 256;

using pb::planck_factor;
using pb::planck_q;
using pb::planck_terms;
using pb::two_stream_down;
using pb::two_stream_trans;
using pb::two_stream_up;

// grid (blocks of 256 columns, walkers): every global access of a wavefront is a contiguous row
// segment.  ec[nw][L][W] is consumed; intervals[nw][L-1], temp[nw][L] -> flux[nw][W].
__global__ __launch_bounds__(kBlock) void k_two_stream_batch(
    double *__restrict__ flux, double *__restrict__ ec, const double *__restrict__ intervals,
    const double *__restrict__ wn, const double *__restrict__ temp,
    const double *__restrict__ f_int, const double *__restrict__ flux_top,
    double *__restrict__ work, int nlayers, int nwave)
{
    // this walker's kKB T [L], its reciprocal [L] and layer intervals [L-1]: wave-uniform reads
    extern __shared__ double s_kt[];
    double *s_h = s_kt + 2 * nlayers;
    const int wk = blockIdx.y;
    for (int k = threadIdx.x; k < nlayers - 1; k += kBlock)
        s_h[k] = intervals[(int64_t)wk * (nlayers - 1) + k];
    planck_terms(s_kt, temp + (int64_t)wk * nlayers, nlayers);        // (ends with the barrier)
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nwave)
        return;
    ec += (int64_t)wk * nlayers * nwave + j;
    work += (int64_t)wk * (nlayers - 1) * nwave + j;
    const double w = wn[j];
    const double factor = planck_factor(w);
    // downward sweep from the irradiation at the top (itop = 0: spectrum.py:498-509)
    double down = flux_top ? flux_top[j] : 0.0;
    double depth = 0.0;
    double prev = ec[0];
    double cur = nlayers > 1 ? ec[nwave] : 0.0;
    double bprev = planck_q(factor, w, s_kt[0], s_kt[nlayers]);
    for (int i = 0; i < nlayers - 1; i++) {
        // (row i + 2 is asked for before this interval's exp1, a row ahead of the stores)
        const double ahead = ec[(int64_t)min(i + 2, nlayers - 1) * nwave];
        // k_plane_depth's running sum without a stop; np.diff(depth): the DIFFERENCE of the sums
        const double dnext = depth + 0.5 * s_h[i] * (cur + prev);
        const double dtau0 = dnext - depth;
        const double trans = two_stream_trans(dtau0);
        const double bnext = planck_q(factor, w, s_kt[i + 1], s_kt[nlayers + i + 1]);
        down = two_stream_down(down, trans, dtau0, bprev, bnext);
        ec[(int64_t)i * nwave] = dtau0;
        work[(int64_t)i * nwave] = trans;
        depth = dnext;
        prev = cur;
        cur = ahead;
        bprev = bnext;
    }
    double up = down + (f_int ? f_int[j] : 0.0);
    // upward sweep; bprev = B[L-1]
    double dtau0 = 0.0, trans = 0.0;
    if (nlayers > 1) {
        dtau0 = ec[(int64_t)(nlayers - 2) * nwave];
        trans = work[(int64_t)(nlayers - 2) * nwave];
    }
    for (int i = nlayers - 2; i >= 0; i--) {
        const int inext = max(i - 1, 0);
        const double dtau_next = ec[(int64_t)inext * nwave];
        const double trans_next = work[(int64_t)inext * nwave];
        const double blo = planck_q(factor, w, s_kt[i], s_kt[nlayers + i]);
        up = two_stream_up(up, trans, dtau0, blo, bprev);
        bprev = blo;
        dtau0 = dtau_next;
        trans = trans_next;
    }
    flux[(int64_t)wk * nwave + j] = up;
}

}  // namespace

extern "C" {

int64_t pb_two_stream_batch_work_doubles(int nlayers, int nwave, int nwalkers)
{
    if (nlayers <= 1 || nwave <= 0 || nwalkers <= 0)
        return 0;
    return (int64_t)nwalkers * (nlayers - 1) * nwave;
}

int pb_two_stream_batch(double *flux_d, double *ec_d, const double *intervals_d,
                        const double *wn_d, const double *temps_d, const double *f_int_d,
                        const double *flux_top_d, double *work_d, int nlayers, int nwave,
                        int nwalkers, void *stream)
{
    PB_REQUIRE(nlayers >= 1 && nwave >= 0 && nwalkers >= 0, "pb_two_stream_batch: bad shape");
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(flux_d && ec_d && wn_d && temps_d && (nlayers == 1 || intervals_d),
               "pb_two_stream_batch: null pointer");
    PB_REQUIRE(work_d || pb_two_stream_batch_work_doubles(nlayers, nwave, nwalkers) == 0,
               "pb_two_stream_batch: null work (pb_two_stream_batch_work_doubles doubles of device "
               "scratch)");
    const size_t lds = ((size_t)3 * nlayers) * sizeof(double);
    PB_REQUIRE(lds <= 64 * 1024, "pb_two_stream_batch: %d layers: at most %d (the walker's "
               "temperatures and intervals are kept in LDS)", nlayers, 64 * 1024 / 24);
    dim3 grid(pb::div_up(nwave, kBlock), nwalkers);
    k_two_stream_batch<<<grid, kBlock, lds, pb::as_stream(stream)>>>(
        flux_d, ec_d, intervals_d, wn_d, temps_d, f_int_d, flux_top_d, work_d, nlayers, nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
