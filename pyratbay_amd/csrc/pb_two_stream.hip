// Two-stream fluxes (pyratbay/pyrat/spectrum.py:454-522; Heng et al. 2014 Eqs. B5-B6; exp1 and the
// statements of one layer interval: pb_two_stream.h), for a batch of walkers and for one spectrum.
//
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
// were recomputed.  The bracket's 1 - exp(-dtau0) (pb_two_stream.h: from expm1) is recomputed on
// the way up (no traffic).
#include "pb_common.h"
#include "pb_planck.h"
#include "pb_two_stream.h"

namespace {

constexpr int kBlock = 256;

using pb::planck;
using pb::planck_factor;
using pb::planck_q;
using pb::planck_terms;
using pb::two_stream_down;
using pb::two_stream_trans;
using pb::two_stream_up;

// The irradiation of a walker with a stellar temperature of its own (pb_two_stream_batch_star):
// the bracket of tstar[walker] in sed_temps[nt], found once per walker (block-uniform).
struct StarTop {
    const double *star_grid;   // [nt][W]; null: the shared flux_top[W] (or none)
    const double *sed_temps;   // [nt]
    const double *tstar;       // [nw]
    double factor;
    int nt;
};

// grid (blocks of 256 columns, walkers): every global access of a wavefront is a contiguous row
// segment.  ec[nw][L][W] is consumed; intervals[nw][L-1], temp[nw][L] -> flux[nw][W].  kStar: the
// top boundary is factor * (the SED grid interpolated at the walker's tstar), interp1d's linear
// rule as SciPy states it (StellarGrid.flux_host) then the multiply, per column in registers; a
// walker whose tstar is NaN or outside the grid reads no grid row and gets a +inf flux row.
template <bool kStar>
__global__ __launch_bounds__(kBlock) void k_two_stream_batch(
    double *__restrict__ flux, double *__restrict__ ec, const double *__restrict__ intervals,
    const double *__restrict__ wn, const double *__restrict__ temp,
    const double *__restrict__ f_int, const double *__restrict__ flux_top, StarTop star,
    double *__restrict__ work, int nlayers, int nwave)
{
    // this walker's kKB T [L], its reciprocal [L] and layer intervals [L-1]: wave-uniform reads
    extern __shared__ double s_kt[];
    double *s_h = s_kt + 2 * nlayers;
    const int wk = blockIdx.y;
    int hi = 1;
    double tstar = 0.0;
    if (kStar) {
        tstar = star.tstar[wk];
        // (block-uniform: every thread of the block leaves here, before any barrier)
        if (!(tstar >= star.sed_temps[0] && tstar <= star.sed_temps[star.nt - 1])) {
            const int j = blockIdx.x * kBlock + threadIdx.x;
            if (j < nwave)
                flux[(int64_t)wk * nwave + j] = INFINITY;
            return;
        }
        // searchsorted(sed_temps, tstar, side='left') clipped to [1, nt - 1]
        hi = 0;
        while (hi < star.nt && star.sed_temps[hi] < tstar)
            hi++;
        hi = min(max(hi, 1), star.nt - 1);
    }
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
    double down;
    if (kStar) {
        const double x_lo = star.sed_temps[hi - 1];
        const double y_lo = star.star_grid[(int64_t)(hi - 1) * nwave + j];
        const double y_hi = star.star_grid[(int64_t)hi * nwave + j];
        const double slope = (y_hi - y_lo) / (star.sed_temps[hi] - x_lo);
        down = star.factor * (slope * (tstar - x_lo) + y_lo);
    } else {
        down = flux_top ? flux_top[j] : 0.0;
    }
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

// ---------------------------------------------------------------------------
// One spectrum: the chain as separate launches over a depth array that k_plane_depth wrote.
// ---------------------------------------------------------------------------

// The diffusivity transmission of every (layer interval, sample), trans[i][j] written to
// flux_up[i][j]: the expensive part of the two-stream solver (exp1: a series or a continued
// fraction of 20 + 80/x terms, one division each) has no dependence between layers, so it gets a
// thread per (interval, sample) instead of sitting in the column sweeps (one thread per column =
// 1.5 wavefronts per SIMD at 1e5 samples).  Same expression as the sweep evaluated before.
__global__ __launch_bounds__(kBlock) void k_two_stream_trans(double *flux_up, const double *depth,
                                                            int nlayers, int nwave)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= nwave || i >= nlayers - 1)
        return;
    const double dtau0 = depth[(int64_t)(i + 1) * nwave + j] - depth[(int64_t)i * nwave + j];
    flux_up[(int64_t)i * nwave + j] = two_stream_trans(dtau0);
}

// One column per thread.  trans[i] comes from k_two_stream_trans (parked in flux_up[i], which
// the upward sweep then overwrites); Planck values are recomputed in registers.
__global__ __launch_bounds__(kBlock) void k_two_stream(
    double *flux_down, double *flux_up, const double *depth, const double *wn,
    const double *temp, const double *f_int, const double *flux_top, int rtop, int nlayers,
    int nwave)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nwave)
        return;
    const double w = wn[j];
    const double factor = planck_factor(w);
    // the irradiation is written into row rtop and the sweep overwrites rows 1..L-1
    // (spectrum.py:498-509): it survives only when rtop == 0
    double down = (flux_top && rtop == 0) ? flux_top[j] : 0.0;
    flux_down[j] = down;
    double dprev = depth[j];
    double bprev = planck(factor, w, temp[0]);
    for (int i = 0; i < nlayers - 1; i++) {
        const double dnext = depth[(int64_t)(i + 1) * nwave + j];
        const double bnext = planck(factor, w, temp[i + 1]);
        const double dtau0 = dnext - dprev;
        const double trans = flux_up[(int64_t)i * nwave + j];
        down = two_stream_down(down, trans, dtau0, bprev, bnext);
        flux_down[(int64_t)(i + 1) * nwave + j] = down;
        dprev = dnext;
        bprev = bnext;
    }
    double up = down + (f_int ? f_int[j] : 0.0);
    flux_up[(int64_t)(nlayers - 1) * nwave + j] = up;
    // bprev = B[L-1], dprev = depth[L-1]
    for (int i = nlayers - 2; i >= 0; i--) {
        const double dlo = depth[(int64_t)i * nwave + j];
        const double blo = planck(factor, w, temp[i]);
        const double dtau0 = dprev - dlo;
        const double trans = flux_up[(int64_t)i * nwave + j];
        up = two_stream_up(up, trans, dtau0, blo, bprev);
        flux_up[(int64_t)i * nwave + j] = up;
        dprev = dlo;
        bprev = blo;
    }
}

// f_int (spectrum.py:475-478): Planck at tint, scaled so that its trapezoid integral over
// wn is sigma*tint^4.  One workgroup; fixed-order tree sum.
__global__ __launch_bounds__(kBlock) void k_internal_flux(double *f_int, const double *wn,
                                                         double tint, int nwave)
{
    __shared__ double s_part[kBlock];
    const double sigma = 5.6703744191844314e-05;      // constants/astrophysical_constants.py:71
    double acc = 0.0;
    for (int i = threadIdx.x; i < nwave; i += kBlock) {
        const double w = wn[i];
        const double b = planck(planck_factor(w), w, tint);
        f_int[i] = b;
        if (i + 1 < nwave) {
            const double w1 = wn[i + 1];
            acc += (w1 - w) * (planck(planck_factor(w1), w1, tint) + b) / 2.0;
        }
    }
    s_part[threadIdx.x] = acc;
    __syncthreads();
    for (int k = kBlock / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k)
            s_part[threadIdx.x] += s_part[threadIdx.x + k];
        __syncthreads();
    }
    const double total = s_part[0];
    if (total > 0) {
        const double scale = sigma * pow(tint, 4.0) / total;
        for (int i = threadIdx.x; i < nwave; i += kBlock)
            f_int[i] *= scale;
    }
}

}  // namespace

extern "C" {

int pb_internal_flux(double *f_int_d, const double *wn_d, double tint, int nwave, void *stream)
{
    PB_REQUIRE(nwave >= 0, "pb_internal_flux: bad shape");
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(f_int_d && wn_d, "pb_internal_flux: null pointer");
    k_internal_flux<<<1, kBlock, 0, pb::as_stream(stream)>>>(f_int_d, wn_d, tint, nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_two_stream(double *flux_down_d, double *flux_up_d, const double *depth_d,
                  const double *wn_d, const double *temp_d, const double *f_int_d,
                  const double *flux_top_d, int rtop, int nlayers, int nwave, void *stream)
{
    PB_REQUIRE(nlayers >= 1 && nwave >= 0, "pb_two_stream: bad shape");
    PB_REQUIRE(rtop >= 0 && rtop < nlayers, "pb_two_stream: rtop out of range");
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(flux_down_d && flux_up_d && depth_d && wn_d && temp_d,
               "pb_two_stream: null pointer");
    if (nlayers > 1) {
        dim3 tgrid((unsigned)pb::div_up(nwave, kBlock), (unsigned)(nlayers - 1));
        k_two_stream_trans<<<tgrid, kBlock, 0, pb::as_stream(stream)>>>(flux_up_d, depth_d,
                                                                         nlayers, nwave);
        PB_LAUNCH_CHECK();
    }
    k_two_stream<<<pb::div_up(nwave, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        flux_down_d, flux_up_d, depth_d, wn_d, temp_d, f_int_d, flux_top_d, rtop, nlayers,
        nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

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
    k_two_stream_batch<false><<<grid, kBlock, lds, pb::as_stream(stream)>>>(
        flux_d, ec_d, intervals_d, wn_d, temps_d, f_int_d, flux_top_d, StarTop{}, work_d, nlayers,
        nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_two_stream_batch_star(double *flux_d, double *ec_d, const double *intervals_d,
                             const double *wn_d, const double *temps_d, const double *f_int_d,
                             const double *star_grid_d, const double *sed_temps_d,
                             const double *tstar_d, double factor, int nt, double *work_d,
                             int nlayers, int nwave, int nwalkers, void *stream)
{
    PB_REQUIRE(nlayers >= 1 && nwave >= 0 && nwalkers >= 0,
               "pb_two_stream_batch_star: bad shape");
    PB_REQUIRE(nt >= 2, "pb_two_stream_batch_star: the grid needs at least 2 temperatures");
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(flux_d && ec_d && wn_d && temps_d && (nlayers == 1 || intervals_d) &&
                   star_grid_d && sed_temps_d && tstar_d,
               "pb_two_stream_batch_star: null pointer");
    PB_REQUIRE(work_d || pb_two_stream_batch_work_doubles(nlayers, nwave, nwalkers) == 0,
               "pb_two_stream_batch_star: null work (pb_two_stream_batch_work_doubles doubles of "
               "device scratch)");
    PB_REQUIRE(nwalkers <= 65535, "pb_two_stream_batch_star: at most 65535 walkers per call");
    const size_t lds = ((size_t)3 * nlayers) * sizeof(double);
    PB_REQUIRE(lds <= 64 * 1024, "pb_two_stream_batch_star: %d layers: at most %d (the walker's "
               "temperatures and intervals are kept in LDS)", nlayers, 64 * 1024 / 24);
    dim3 grid(pb::div_up(nwave, kBlock), nwalkers);
    k_two_stream_batch<true><<<grid, kBlock, lds, pb::as_stream(stream)>>>(
        flux_d, ec_d, intervals_d, wn_d, temps_d, f_int_d, nullptr,
        StarTop{star_grid_d, sed_temps_d, tstar_d, factor, nt}, work_d, nlayers, nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
