// Transit geometry for ONE spectrum: optical depth along the rays of every impact parameter, the
// reference's early exit and the transmission integral.  A thread owns a column: the
// [layer][wavenumber] arrays are row-major so that the 64 lanes of a wavefront read 512 contiguous
// bytes of one layer and walk down the layers; per-layer scalars (ray paths, radii) are
// wave-uniform and come through the scalar cache or LDS.  (The walker batch: pb_transit.hip.)
//
// Reference functions restated (pyratbay v2.0.1): src_c/_trapezoid.c:238-276 and the Python loops
// pyratbay/opacity/optic_depth.py:103-112, pyratbay/spectrum/radiative_transfer.py:57-71.
#include <algorithm>
#include <cstdlib>

#include "pb_common.h"
#include "pb_transit.h"

namespace {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------
// _trapezoid.optdepth: one impact parameter (src_c/_trapezoid.c:238-276)
// ---------------------------------------------------------------------------
__global__ void k_optdepth(double *tau, const double *data, int64_t row_stride,
                           const double *h, int nint, double taumax, int32_t *ideep,
                           int ilay, int nwave)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nwave)
        return;
    double acc = 0.0;
    if (ideep[j] < 0) {
        double prev = nint > 0 ? data[j] : 0.0;
        for (int i = 0; i < nint; i++) {
            double next = data[(int64_t)(i + 1) * row_stride + j];
            acc += h[i] * (next + prev);
            prev = next;
        }
        if (acc > taumax)
            ideep[j] = ilay;
    }
    tau[j] = acc;
}

// ---------------------------------------------------------------------------
// Transit optical depth for all impact parameters (optic_depth.py:103-112), two kernels.
//
// k_transit_tau: thread = (column, block of kRowsPerThread impact parameters).  The
// column of ec is streamed once per row block (coalesced over columns, served by L2 after
// the first block), the kRowsPerThread running sums stay in registers and the ray-path
// segments are wave-uniform scalar loads.  tau_r = sum_{i<r} path_r[i]*(ec[i+1]+ec[i])
// is accumulated in the reference's order (same products, same additions), for EVERY row.
//
// k_transit_finish: thread = column.  Walks the rows once: finds the first crossing of
// maxdepth (the reference's early exit), zeroes the rows below it, writes ideep
// (including the final `ideep[ideep<0] = r`) and, when asked, integrates the
// transmission spectrum exp(-tau)*r over the rows down to ideep
// (radiative_transfer.py:57-71) in the same pass.
// ---------------------------------------------------------------------------
constexpr int kRowsPerThread = 16;     // 32 and 40 measured slower at W = 1e5
// Narrow grids (a wavenumber shard of a multi-GPU run: 12 500 columns) do not fill the chip
// with one thread per (column, 16 rows): they take 4 rows per thread and 64-thread workgroups.
constexpr int kRowsPerThreadNarrow = 4;
constexpr int kNarrowColumns = 32768;

// kScalar: `raypath` is the blocked layout of pb_path_blocks_launch ([block][segment][row], zero
// where segment >= row) and is read through the constant address space = scalar loads, the
// products taking the path from SGPRs; else the packed triangle, staged per block in LDS.
template <int kRows, bool kScalar>
__global__ __launch_bounds__(kBlock) void k_transit_tau(double *depth, const double *ec,
                                                        const double *raypath, int itop,
                                                        int ibottom, int nlayers, int nwave)
{
    // ray-path segments of this block's rows, [segment i][row k], zero where i >= r:
    // adding 0 * s leaves a sum unchanged, so one predicate-free loop serves all rows
    extern __shared__ __align__(16) double s_path[];
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    const int nrow = nlayers - itop;
    const int nimpact = min(ibottom, nlayers) - itop;     // rows 0..nimpact-1 are evaluated
    const int rb = blockIdx.y * kRows;
    const int rlast = min(rb + kRows, nimpact) - 1;       // last evaluated row here
    const int nseg = rb < nimpact ? max(rlast, 0) : 0;    // segments i < rlast; none below ibottom
    if (!kScalar) {
        for (int e = threadIdx.x; e < nseg * kRows; e += blockDim.x) {
            const int i = e / kRows, k = e % kRows;
            const int r = rb + k;
            s_path[e] = (r <= rlast && i < r) ? raypath[(r * (r - 1)) / 2 + i] : 0.0;
        }
        __syncthreads();
    }
    if (col >= nwave)
        return;
    double tau[kRows];
#pragma unroll
    for (int k = 0; k < kRows; k++)
        tau[k] = 0.0;
    if (nseg > 0) {
        const double *src = ec + (int64_t)itop * nwave + col;
        double prev = src[0];
        if (kScalar) {
            // blocks before this one are full: nseg_b = kRows*b + kRows - 1
            const int64_t b = blockIdx.y;
            const int64_t boff = (int64_t)kRows * (kRows * b * (b - 1) / 2 + b * (kRows - 1));
            typedef const double __attribute__((address_space(4))) *cpath_t;
            const cpath_t pb_ = (cpath_t)(unsigned long long)(raypath + boff);
            // rows of ec are fetched kAhead at a time, one group ahead of the sums that use them
            constexpr int kAhead = 4;
            double nx[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; j++)
                nx[j] = src[(int64_t)min(j + 1, nseg) * nwave];
            for (int i0 = 0; i0 < nseg; i0 += kAhead) {
                double cur[kAhead];
#pragma unroll
                for (int j = 0; j < kAhead; j++)
                    cur[j] = nx[j];
#pragma unroll
                for (int j = 0; j < kAhead; j++)
                    nx[j] = src[(int64_t)min(i0 + kAhead + j + 1, nseg) * nwave];
#pragma unroll
                for (int j = 0; j < kAhead; j++) {
                    const int i = i0 + j;
                    if (i < nseg) {                             // uniform
                        const double s = cur[j] + prev;
                        prev = cur[j];
                        double pv[kRows];
#pragma unroll
                        for (int k = 0; k < kRows; k++)
                            pv[k] = pb_[i * kRows + k];
#pragma unroll
                        for (int k = 0; k < kRows; k++)
                            tau[k] += pv[k] * s;
                    }
                }
            }
        } else {
#pragma unroll 4
            for (int i = 0; i < nseg; i++) {
                const double next = src[(int64_t)(i + 1) * nwave];
                const double s = next + prev;
                prev = next;
                const double *pk = s_path + i * kRows;          // LDS broadcast reads
#pragma unroll
                for (int k = 0; k < kRows; k++)
                    tau[k] += pk[k] * s;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kRows; k++) {
        const int r = rb + k;
        if (r < nrow)
            depth[(int64_t)(itop + r) * nwave + col] = tau[k];     // 0 for r >= nimpact
    }
    if (blockIdx.y == 0)
        for (int r = 0; r < itop; r++)
            depth[(int64_t)r * nwave + col] = 0.0;
}

// Opaque cloud deck (radiative_transfer.py:62-66): at row deck_row = deck_itop - itop the
// interval's far end is the cloud top: h = rsurf - radius[deck_itop-1] and the integrand is
// the linear interpolation (scipy interp1d) of exp(-tau)*r between the two layers at rsurf.
using pb::deck_integrand;         // (pb_common.h)

__global__ __launch_bounds__(kBlock) void k_transit_finish(
    double *depth, int32_t *ideep, double *spectrum, const double *radius_g, double rstar,
    int itop, int ibottom, double maxdepth, int nlayers, int nwave, int deck_row, double rsurf)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= nwave)
        return;
    // the radii are wave-uniform: scalar loads through the constant address space (as
    // same-address vector loads they sit in the dependent chain of every row)
    typedef const double __attribute__((address_space(4))) *crad_t;
    const crad_t radius = (crad_t)(unsigned long long)radius_g;
    const int nimpact = min(ibottom, nlayers) - itop;
    int stop = -1;
    double acc = 0.0, fprev = 0.0, rprev = 0.0;
    // rows are fetched eight at a time (independent loads in flight), then examined in order
    constexpr int kFetch = 8;
    double nx[kFetch];
#pragma unroll
    for (int k = 0; k < kFetch; k++)
        nx[k] = k < nimpact ? depth[(int64_t)(itop + k) * nwave + col] : 0.0;
    for (int r0 = 0; r0 < nimpact; r0 += kFetch) {
        double t[kFetch];
#pragma unroll
        for (int k = 0; k < kFetch; k++)
            t[k] = nx[k];
        // the next group is requested before this one is examined
#pragma unroll
        for (int k = 0; k < kFetch; k++)
            nx[k] = (r0 + kFetch + k < nimpact)
                        ? depth[(int64_t)(itop + r0 + kFetch + k) * nwave + col]
                        : 0.0;
#pragma unroll
        for (int k = 0; k < kFetch; k++) {
            const int r = r0 + k;
            if (r >= nimpact)
                break;
            if (stop < 0) {
                if (spectrum) {
                    const double rad = radius[itop + r];
                    double f = pb::exp_s(-t[k]) * rad;
                    if (r > 0 && r == deck_row) {
                        f = deck_integrand(fprev, f, rprev, rad, rsurf);
                        acc += (rsurf - rprev) * (fprev + f);
                    } else if (r > 0) {
                        acc += (rad - rprev) * (fprev + f);
                    }
                    fprev = f;
                    rprev = rad;
                }
                if (t[k] > maxdepth)
                    stop = r;
            } else if (t[k] != 0.0) {
                depth[(int64_t)(itop + r) * nwave + col] = 0.0;   // below the first crossing
            }
        }
    }
    // ideep[ideep<0] = r with r the last loop value (itop if the loop is empty)
    const int last = nimpact > 0 ? itop + nimpact - 1 : itop;
    ideep[col] = stop >= 0 ? itop + stop : last;
    if (spectrum) {
        const double rtop = radius[itop];
        spectrum[col] = (rtop * rtop + 2 * (acc * 0.5)) / (rstar * rstar);
    }
}

// ---------------------------------------------------------------------------
// Fused transmission spectrum (radiative_transfer.py:57-71, no cloud deck)
// ---------------------------------------------------------------------------
__global__ void k_transmission(double *spectrum, const double *depth,
                               const int32_t *ideep, const double *radius, int itop,
                               double rstar, int nlayers, int nwave, int deck_row, double rsurf)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nwave)
        return;
    int n = ideep[j] - itop;                 // number of intervals
    if (n > nlayers - 1 - itop)
        n = nlayers - 1 - itop;
    double acc = 0.0;
    if (n > 0) {
        double rprev = radius[itop];
        double prev = pb::exp_s(-depth[(int64_t)itop * nwave + j]) * rprev;
        for (int i = 0; i < n; i++) {
            double rnext = radius[itop + i + 1];
            double next = pb::exp_s(-depth[(int64_t)(itop + i + 1) * nwave + j]) * rnext;
            if (i + 1 == deck_row) {
                next = deck_integrand(prev, next, rprev, rnext, rsurf);
                acc += (rsurf - rprev) * (prev + next);
            } else {
                acc += (rnext - rprev) * (prev + next);
            }
            prev = next;
            rprev = rnext;
        }
    }
    acc *= 0.5;
    double rtop = radius[itop];
    spectrum[j] = (rtop * rtop + 2 * acc) / (rstar * rstar);
}

// ---------------------------------------------------------------------------
// one transit launch: environment, plan, ray-path layout, then the kernels of the planned form
// ---------------------------------------------------------------------------

// The PB_* variables a launch consults.  Read once at the top of EVERY launch, never kept in a
// static: the tests change them between calls of one process.
struct TransitOneTuning {
    bool fused = false;            // PB_TRANSIT=fused: pb_transit.hip's one-pass kernel (split: the default)
    bool no_scalar = false;        // PB_TRANSIT_SCALAR=0: ray paths staged in LDS
};

TransitOneTuning read_transit_one_tuning()
{
    TransitOneTuning t;
    if (const char *e = getenv("PB_TRANSIT"))
        t.fused = !strcmp(e, "fused");
    if (const char *e = getenv("PB_TRANSIT_SCALAR"))
        t.no_scalar = atoi(e) == 0;
    return t;
}

// What a launch will run, decided from the shape and the environment alone.
enum class TransitOneForm {
    Fused,         // pb_transit_fused_launch with one walker (PB_TRANSIT=fused; tests compare the forms)
    Split,         // k_transit_tau for every row, then k_transit_finish
    Refused,       // Split, but a block's ray paths do not fit in LDS
};

struct TransitOnePlan {
    TransitOneForm form = TransitOneForm::Split;
    int rows = 0;                    // impact parameters per thread of k_transit_tau
    int threads = 0;                 // per workgroup, of both kernels
    dim3 grid;                       // of k_transit_tau: (blocks of columns, blocks of rows)
    size_t lds = 0;                  // dynamic LDS bytes of k_transit_tau<rows, false>
    bool build_path_blocks = false;  // re-lay the ray paths for k_transit_tau<rows, true>
    int deck_row = -1;               // row of an opaque cloud deck below itop, or none
};

// nrow = nlayers - itop rows of depth, of which the first nimpact are evaluated
TransitOnePlan plan_transit_one(int nrow, int nimpact, int nwave, int itop, int deck_itop,
                                const TransitOneTuning &tn, bool capturing)
{
    TransitOnePlan p;
    // radiative_transfer.py:63: the deck matters only when it lies below the top layer
    p.deck_row = deck_itop > itop ? deck_itop - itop : -1;
    // One spectrum: two kernels (tau for every row with grid.y over blocks of impact parameters,
    // then the early exit): a single grid of columns has too few wavefronts for the fused
    // one-pass kernel of pb_transit.hip (C2: 155 us fused against 97 us), which is what the
    // walker-batched path uses.  PB_TRANSIT=fused|split forces one form (tests compare them).
    if (tn.fused) {
        p.form = TransitOneForm::Fused;
        return p;
    }
    const bool narrow = nwave <= kNarrowColumns;
    p.rows = narrow ? kRowsPerThreadNarrow : kRowsPerThread;
    p.threads = narrow ? 64 : kBlock;
    p.grid = dim3(pb::div_up(nwave, p.threads), pb::div_up(nrow, p.rows));
    // (the LDS form must stay possible: it is what a launch falls back to)
    p.lds = (size_t)nrow * p.rows * sizeof(double);
    if (p.lds > 64 * 1024) {
        p.form = TransitOneForm::Refused;
        return p;
    }
    // the ray paths re-laid per block of rows in the stream's scratch, so that the kernel can
    // take them with scalar loads (PB_TRANSIT_SCALAR=0: packed triangle staged in LDS)
    // (not while the stream is being captured: a graph must not depend on scratch that other work
    // on a stream of the same handle may overwrite when the graph is replayed elsewhere)
    p.build_path_blocks = !tn.no_scalar && nimpact > 1 && !capturing;
    return p;
}

int transit_launch(double *depth_d, int32_t *ideep_d, double *spectrum_d, const double *ec_d,
                   const double *raypath_d, const double *radius_d, double rstar, int itop,
                   int ibottom, double maxdepth, int nlayers, int nwave, void *stream,
                   const char *who, int deck_itop = -1, double deck_rsurf = 0.0)
{
    PB_REQUIRE(nlayers > 0 && nwave >= 0, "%s: bad shape", who);
    PB_REQUIRE(itop >= 0 && itop < nlayers, "%s: itop out of range", who);
    PB_REQUIRE(ibottom <= nlayers, "%s: ibottom > nlayers", who);
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(depth_d && ideep_d && ec_d, "%s: null pointer", who);
    const int nrow = nlayers - itop;
    PB_REQUIRE(nrow == 1 || raypath_d, "%s: null raypath", who);
    PB_REQUIRE(!spectrum_d || radius_d, "%s: null radius", who);
    const hipStream_t s = pb::as_stream(stream);
    const int nimpact = std::min(ibottom, nlayers) - itop;
    const int64_t npath = ((int64_t)nrow * (nrow - 1)) / 2;

    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &capturing) != hipSuccess)
        (void)hipGetLastError();
    const TransitOnePlan p =
        plan_transit_one(nrow, nimpact, nwave, itop, deck_itop, read_transit_one_tuning(),
                         capturing != hipStreamCaptureStatusNone);

    if (p.form == TransitOneForm::Fused) {
        TransitCall c;
        c.depth = depth_d;
        c.ideep = ideep_d;
        c.spectrum = spectrum_d;
        c.ec = ec_d;
        c.raypath = raypath_d;
        c.radius = radius_d;
        c.npath = npath;
        c.rstar = rstar;
        c.itop = itop;
        c.ibottom = ibottom;
        c.maxdepth = maxdepth;
        c.nlayers = nlayers;
        c.nwave = nwave;
        c.nwalkers = 1;
        c.deck_row = p.deck_row;
        c.rsurf = deck_rsurf;
        return pb_transit_fused_launch(c, s);
    }
    if (p.form == TransitOneForm::Refused) {
        pb::set_error("%s: %d layers need %zu B of LDS", who, nrow, p.lds);
        return PB_ERR_UNSUPPORTED;
    }

    double *blocked = nullptr;
    if (p.build_path_blocks) {
        int64_t plen = 0;
        if (pb_path_blocks_launch(&blocked, &plen, raypath_d, npath, p.rows, nimpact, s) != PB_OK)
            blocked = nullptr;                     // fall back to the LDS form
    }
    const bool scalar = blocked != nullptr;
    const double *path = scalar ? blocked : raypath_d;
    const size_t lds = scalar ? 0 : p.lds;
    switch (p.rows * 2 + scalar) {
    case kRowsPerThreadNarrow * 2 + 1:
        k_transit_tau<kRowsPerThreadNarrow, true><<<p.grid, p.threads, lds, s>>>(
            depth_d, ec_d, path, itop, ibottom, nlayers, nwave);
        break;
    case kRowsPerThreadNarrow * 2:
        k_transit_tau<kRowsPerThreadNarrow, false><<<p.grid, p.threads, lds, s>>>(
            depth_d, ec_d, path, itop, ibottom, nlayers, nwave);
        break;
    case kRowsPerThread * 2 + 1:
        k_transit_tau<kRowsPerThread, true><<<p.grid, p.threads, lds, s>>>(
            depth_d, ec_d, path, itop, ibottom, nlayers, nwave);
        break;
    default:
        k_transit_tau<kRowsPerThread, false><<<p.grid, p.threads, lds, s>>>(
            depth_d, ec_d, path, itop, ibottom, nlayers, nwave);
        break;
    }
    PB_LAUNCH_CHECK();
    // end of the reference's 'odepth' stage when this call also integrates the spectrum (the
    // finish pass resolves the early exit AND integrates: it is counted as 'spectrum')
    if (spectrum_d)
        pb::stage_boundary("odepth", "spectrum", s);
    k_transit_finish<<<pb::div_up(nwave, p.threads), p.threads, 0, s>>>(
        depth_d, ideep_d, spectrum_d, radius_d, rstar, itop, ibottom, maxdepth, nlayers, nwave,
        p.deck_row, deck_rsurf);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int pb_optdepth(double *tau_d, const double *data_d, int64_t row_stride,
                const double *intervals_d, int nint, double taumax, int32_t *ideep_d,
                int ilay, int nwave, void *stream)
{
    PB_REQUIRE(nwave >= 0 && nint >= 0, "pb_optdepth: negative size");
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(tau_d && data_d && ideep_d && (nint == 0 || intervals_d),
               "pb_optdepth: null pointer");
    PB_REQUIRE(row_stride >= nwave, "pb_optdepth: row_stride < nwave");
    k_optdepth<<<pb::div_up(nwave, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        tau_d, data_d, row_stride, intervals_d, nint, taumax, ideep_d, ilay, nwave);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_optical_depth_transit(double *depth_d, int32_t *ideep_d, const double *ec_d,
                             const double *raypath_d, int itop, int ibottom,
                             double maxdepth, int nlayers, int nwave, void *stream)
{
    return transit_launch(depth_d, ideep_d, nullptr, ec_d, raypath_d, nullptr, 1.0, itop,
                          ibottom, maxdepth, nlayers, nwave, stream,
                          "pb_optical_depth_transit");
}

int pb_transit_spectrum(double *spectrum_d, double *depth_d, int32_t *ideep_d,
                        const double *ec_d, const double *raypath_d, const double *radius_d,
                        double rstar, int itop, int ibottom, double maxdepth, int nlayers,
                        int nwave, void *stream)
{
    PB_REQUIRE(spectrum_d, "pb_transit_spectrum: null spectrum");
    return transit_launch(depth_d, ideep_d, spectrum_d, ec_d, raypath_d, radius_d, rstar, itop,
                          ibottom, maxdepth, nlayers, nwave, stream, "pb_transit_spectrum");
}

int pb_transit_spectrum_deck(double *spectrum_d, double *depth_d, int32_t *ideep_d,
                             const double *ec_d, const double *raypath_d,
                             const double *radius_d, double rstar, int itop, int ibottom,
                             double maxdepth, int deck_itop, double deck_rsurf, int nlayers,
                             int nwave, void *stream)
{
    PB_REQUIRE(spectrum_d, "pb_transit_spectrum_deck: null spectrum");
    PB_REQUIRE(deck_itop < nlayers, "pb_transit_spectrum_deck: deck_itop out of range");
    return transit_launch(depth_d, ideep_d, spectrum_d, ec_d, raypath_d, radius_d, rstar, itop,
                          ibottom, maxdepth, nlayers, nwave, stream,
                          "pb_transit_spectrum_deck", deck_itop, deck_rsurf);
}

int pb_transmission_deck(double *spectrum_d, const double *depth_d, const int32_t *ideep_d,
                         const double *radius_d, int itop, double rstar, int deck_itop,
                         double deck_rsurf, int nlayers, int nwave, void *stream)
{
    PB_REQUIRE(nlayers > 0 && nwave >= 0, "pb_transmission: bad shape");
    PB_REQUIRE(itop >= 0 && itop < nlayers, "pb_transmission: itop out of range");
    PB_REQUIRE(deck_itop < nlayers, "pb_transmission: deck_itop out of range");
    if (nwave == 0)
        return PB_OK;
    PB_REQUIRE(spectrum_d && depth_d && ideep_d && radius_d, "pb_transmission: null pointer");
    const int deck_row = deck_itop > itop ? deck_itop - itop : -1;
    k_transmission<<<pb::div_up(nwave, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        spectrum_d, depth_d, ideep_d, radius_d, itop, rstar, nlayers, nwave, deck_row,
        deck_rsurf);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_transmission(double *spectrum_d, const double *depth_d, const int32_t *ideep_d,
                    const double *radius_d, int itop, double rstar, int nlayers,
                    int nwave, void *stream)
{
    return pb_transmission_deck(spectrum_d, depth_d, ideep_d, radius_d, itop, rstar, -1, 0.0,
                                nlayers, nwave, stream);
}

}  // extern "C"
