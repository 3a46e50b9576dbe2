// Cloud deck and patchy clouds in the walker-batched retrieval path (TableSpectrum.eval_bands with
// deck_logp / f_patchy).
//
// The reference evaluates a patchy model as TWO atmospheres (opacity/optic_depth.py:94-136): the
// clear one, ec over all layers, and the cloudy one, ec + ec_cloud from itop down to the opaque
// deck (opacity/clouds/gray.py:95-154 sets deck_itop, rsurf, tsurf; pyrat_obj.py:135-139 cuts the
// optical-depth integration at deck_itop + 1; spectrum/radiative_transfer.py:63-67, 125-127 puts
// the deck at the bottom of the radiative transfer), then mixes the two spectra
// (pyrat/spectrum.py:357-363, 378-384).  Here both columns of a walker come out of ONE pass over
// its ec, and ec + ec_cloud is never stored (a second ec[nw, L, W] is 4.1 GB per 64 walkers at
// C5's shape):
//   * ec_cloud is a sum of rank-1 terms cs_m[sample] f_m[walker, layer] (Lecavelier, CCSgray): a
//     thread keeps the cs_m of its sample in registers and adds sum_m cs_m f_m as it walks
//     (pb::CloudWalk; kTwo: two running sums side by side);
//   * with the deck as the only cloud-type model ec_cloud is zero: the optical depths of the two
//     columns are equal row for row down to the deck, so one running sum serves both and the
//     cloudy column is closed on the way (at its crossing of maxdepth if that comes first, else at
//     the deck).
// Per column the arithmetic does not depend on where the column sits: grid order and any column
// order give the same bits.  The walk itself -- the cloudy column, the patchy mix, the transit
// blocks of impact parameters -- is stated in pb_cloud_walk.h, for these kernels and for the band
// contribution kernels (pb_contribution.hip).
//
//   k_deck_state       (deck_itop, rsurf, tsurf) of every walker from its log10 pressure
//   k_cloud_plan/rows  the rank-1 factors of the cloud-type models from the walkers' parameters
//   k_cloudy_transit   ec -> transit spectrum  f cloudy + (1 - f) clear
//   k_cloudy_emission  ec -> emission flux     f cloudy + (1 - f) clear
#include <algorithm>

#include "pb_cloud_walk.h"
#include "pb_common.h"
#include "pb_planck.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxMu = 16;
constexpr int kMaxCloud = PB_CLOUD_MAX;          // (the plan's; the terms' cap: pb_cloud_walk.h)
constexpr double kBar = 1e6, kBoltz = 1.380649e-16;   // the continuum models' units (lecavelier.py)

using pb::cdbl_t;
using pb::CloudWalk;
using pb::uniform_f64;
using pb::planck_factor;
using pb::planck_q;
using pb::planck_terms;

// ---------------------------------------------------------------------------
// Deck.calc_extinction_coefficient per walker (gray.py:129-150): itop by the reference's rule,
// rsurf and tsurf by np.interp's arithmetic (slope * (x - x_lo) + y_lo, a value on a node taken
// unchanged, the end values outside the grid).
// ---------------------------------------------------------------------------
__device__ inline double interp_clamped(const double *xp, const double *fp, int n, double x)
{
    if (x > xp[n - 1])
        return fp[n - 1];
    if (x < xp[0])
        return fp[0];
    int lo = 0, hi = n - 1;                    // largest lo with xp[lo] <= x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (xp[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    if (xp[hi] <= x)
        lo = hi;
    if (lo == n - 1 || xp[lo] == x)
        return fp[lo];
    const double slope = (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo]);
    return slope * (x - xp[lo]) + fp[lo];
}

__global__ __launch_bounds__(kBlock) void k_deck_state(
    int32_t *itop, double *rsurf, double *tsurf, const double *pressure, const double *logp,
    const double *radius, int64_t radius_stride, const double *temps, int nlayers, int nwalkers)
{
    const int w = blockIdx.x * kBlock + threadIdx.x;
    if (w >= nwalkers)
        return;
    const double p = pow(10.0, logp[w]);
    int it;
    if (p >= pressure[nlayers - 1]) {
        it = nlayers - 1;
    } else if (p < pressure[0]) {
        it = 1;
    } else {
        int lo = 0, hi = nlayers - 1;          // first layer with pressure >= p (NaN: the last)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (pressure[mid] >= p)
                hi = mid;
            else
                lo = mid + 1;
        }
        it = lo;
    }
    itop[w] = min(it, nlayers - 1);
    if (p != p) {
        rsurf[w] = tsurf[w] = p;
        return;
    }
    rsurf[w] = interp_clamped(pressure, radius + (int64_t)w * radius_stride, nlayers, p);
    tsurf[w] = interp_clamped(pressure, temps + (int64_t)w * nlayers, nlayers, p);
}

// ---------------------------------------------------------------------------
// The factors of the cloud-type rank-1 models, with the expressions of k_cont_plan / k_cont_rows
// (pb_interp_cont.hip), which form the same models when they go into ec.
// ---------------------------------------------------------------------------
struct PlanArgs {
    double *f, *rows;
    const double *temps, *pars, *wn;
    int pars_stride, nlayers, nwave, nwalkers;
    pb_cloud_models m;
};

__global__ __launch_bounds__(kBlock) void k_cloud_plan(PlanArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)a.nwalkers * a.nlayers)
        return;
    const int l = (int)(i % a.nlayers);
    const int64_t w = i / a.nlayers;
    const double t = a.temps[i];
    const double *p = a.pars + w * a.pars_stride;
    for (int m = 0; m < a.m.nr; m++) {
        const double pr = a.m.pressure_d[m][l];
        const double nominal = pr * kBar / t / kBoltz;
        double f = nominal;
        if (a.m.kind[m] == 2) {
            const int q = a.m.par[m];
            const double p_top = pow(10.0, p[q + 2]), p_bottom = pow(10.0, p[q + 1]);
            const double cs = pr >= p_bottom && pr <= p_top ? pow(10.0, p[q]) * a.m.s0[m] : 0.0;
            f = cs * nominal;
        }
        a.f[i * a.m.nr + m] = f;
    }
}

// Lecavelier.calc_cross_section per walker: 10**p0 * s0 * (wn * l0)**(-p1); blockIdx.z = model
__global__ __launch_bounds__(kBlock) void k_cloud_rows(PlanArgs a)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int w = blockIdx.y;
    if (i >= a.nwave)
        return;
    int m = 0;
    for (int j = -1; m < a.m.nr; m++)
        if (a.m.kind[m] == 1 && ++j == (int)blockIdx.z)
            break;
    const double *p = a.pars + (int64_t)w * a.pars_stride + a.m.par[m];
    a.rows[((int64_t)blockIdx.z * a.nwalkers + w) * a.nwave + i] =
        pow(10.0, p[0]) * a.m.s0[m] * pow(a.wn[i] * a.m.l0[m], -p[1]);
}

// ---------------------------------------------------------------------------
// What the two column kernels share
// ---------------------------------------------------------------------------
struct CloudArgs {
    double *spectrum, *clear, *cloudy;         // [nwalkers][nwave], grid order; clear/cloudy or null
    const double *ec;
    const int32_t *column;                     // grid index of each column of ec, or null
    const int32_t *deck_itop;                  // [nwalkers] or null: no deck
    const double *deck_surf;                   // [nwalkers]: rsurf (transit) / tsurf (emission)
    const double *f_patchy;                    // [nwalkers] or null: the cloudy column alone
    double maxdepth;
    int itop, nlayers, nwave;
    pb_cloud_terms cl;
};

// spectrum = f cloudy + (1 - f) clear (pyrat/spectrum.py:362, 384), scattered to grid order
__device__ __forceinline__ void cloud_store(const CloudArgs &a, int w, int col, double clear,
                                            double cloudy)
{
    double out = cloudy;
    if (a.f_patchy)
        out = pb::patchy_mix(pb::patchy_fraction(a.f_patchy, w), cloudy, clear);
    const int dst = a.column ? a.column[col] : col;
    if (dst < 0 || dst >= a.nwave)
        return;
    const int64_t o = (int64_t)w * a.nwave + dst;
    a.spectrum[o] = out;
    if (a.clear)
        a.clear[o] = clear;
    if (a.cloudy)
        a.cloudy[o] = cloudy;
}

// ---------------------------------------------------------------------------
// Transit: the pass of k_transit_fused (pb_transit.hip; optic_depth.py:103-112 with the early exit
// of _trapezoid.c:259-273, radiative_transfer.py:57-71) for the two columns of a walker.
// thread = column; the impact parameters are taken kRows at a time, the ray-path segments of the
// block staged in LDS ([segment][row], zero where segment >= row).  kTwo: ec_cloud != 0, the
// cloudy column has optical depths of its own; else the rows of one sum serve both columns.
// Row r of the cloudy column exists for r < deck_itop + 1 - itop; its last interval ends at the
// deck's radius (deck_integrand, as in k_transit_fused).  The staging and the rows' optical
// depths are pb::stage_path_block / pb::depth_block.
// ---------------------------------------------------------------------------
struct TransitGeom {
    const double *raypath, *radius;
    int64_t path_stride, radius_stride;
    double rstar;
};

using pb::deck_integrand;         // (pb_common.h)

template <int kRows, bool kTwo>
__global__ __launch_bounds__(kBlock) void k_cloudy_transit(CloudArgs a, TransitGeom g)
{
    extern __shared__ __align__(16) double s_path[];      // [segment][kRows]
    const int w = blockIdx.y;
    const int col = blockIdx.x * kBlock + threadIdx.x;
    const bool active = col < a.nwave;
    const int nlayers = a.nlayers, nwave = a.nwave, itop = a.itop;
    const double *path = g.raypath + (int64_t)w * g.path_stride;
    const cdbl_t rad = (cdbl_t)(unsigned long long)(g.radius + (int64_t)w * g.radius_stride);
    const bool deck = a.deck_itop != nullptr;
    const bool need_clear = a.f_patchy || a.clear;
    // wave-uniform: the walker's deck
    const int dk = deck ? pb::deck_layer(a.deck_itop, w, nlayers) : -1;
    const double rsurf = deck ? uniform_f64(a.deck_surf + w) : 0.0;
    const int nimp_c = (deck ? dk + 1 : nlayers) - itop;  // rows of the cloudy column (<= 0: none)
    const int nimp_l = need_clear ? nlayers - itop : 0;
    const int nimp = max(nimp_c, nimp_l);
    const int deck_row = deck ? dk - itop : -1;
    const double *src = a.ec + ((int64_t)w * nlayers + itop) * nwave + (active ? col : 0);
    CloudWalk cloud;
    if (kTwo)
        cloud.init(a.cl, w, active ? col : 0, nlayers);

    bool open_l = nimp_l > 0, open_c = nimp_c > 0;
    double acc_l = 0.0, acc_c = 0.0, fprev_l = 0.0, fprev_c = 0.0;
    for (int rb = 0; rb < nimp; rb += kRows) {
        // every column of the workgroup has closed both of its integrals: nothing left to compute
        if (__syncthreads_count(active && (open_l || open_c)) == 0)
            break;
        const int rlast = min(rb + kRows, nimp) - 1;
        pb::stage_path_block<kRows, kBlock>(s_path, path, rb, rlast);
        __syncthreads();
        if (!active || !(open_l || open_c))
            continue;
        double tau[kRows], tau_c[kTwo ? kRows : 1];
        pb::depth_block<kRows, kTwo>(tau, tau_c, src, nwave, rlast, s_path, cloud, itop);
#pragma unroll
        for (int k = 0; k < kRows; k++) {
            const int r = rb + k;
            if (r > rlast)
                continue;
            const double rr = rad[itop + r];
            const double rprev = r > 0 ? rad[itop + r - 1] : 0.0;
            const double t = tau[k];
            const double t_c = kTwo ? tau_c[k] : t;
            const bool do_l = open_l && r < nimp_l, do_c = open_c && r < nimp_c;
            double f = 0.0;
            if (do_l || (!kTwo && do_c))
                f = pb::exp_s(-t) * rr;
            if (do_l) {
                if (r > 0)
                    acc_l += (rr - rprev) * (fprev_l + f);
                fprev_l = f;
                if (t > a.maxdepth)
                    open_l = false;
            }
            if (do_c) {
                double fc = kTwo ? pb::exp_s(-t_c) * rr : f;
                if (r > 0 && r == deck_row) {
                    fc = deck_integrand(fprev_c, fc, rprev, rr, rsurf);
                    acc_c += (rsurf - rprev) * (fprev_c + fc);
                } else if (r > 0) {
                    acc_c += (rr - rprev) * (fprev_c + fc);
                }
                fprev_c = fc;
                if (t_c > a.maxdepth || r == nimp_c - 1)
                    open_c = false;
            }
        }
    }
    if (!active)
        return;
    const double rtop = rad[itop];
    const double clear = (rtop * rtop + 2 * (acc_l * 0.5)) / (g.rstar * g.rstar);
    const double cloudy = (rtop * rtop + 2 * (acc_c * 0.5)) / (g.rstar * g.rstar);
    cloud_store(a, w, col, clear, cloudy);
}

// ---------------------------------------------------------------------------
// Emission: the pass of k_emission_fused (pb_emission.hip; _trapezoid.c:175-213, 304-341 +
// pyrat/spectrum.py:366-377) for the two columns.  The walker's Planck terms hold the deck's
// temperature in row deck_itop for BOTH columns (the reference's cloudy pass writes that row of its
// Planck array in place and the clear pass reads the array afterwards).  The cloudy column's
// deepest layer is deck_itop (np.clip(ideep, 0, deck_itop), radiative_transfer.py:127).
// ---------------------------------------------------------------------------
struct EmissionGeom {
    const double *intervals, *wn, *temp, *mu, *weights;
    int nmu;
};

template <int MU>
__device__ __forceinline__ double emission_total(double blast, double tlast,
                                                 const double (&acc)[MU], int last, int rtop,
                                                 const EmissionGeom &g, const double *s_imu)
{
    double total = 0.0;
#pragma unroll
    for (int m = 0; m < MU; m++) {
        if (m < g.nmu) {
            double val;
            if (last - rtop == 1)
                val = blast;
            else
                val = blast * pb::exp_s(pb::quot_fast(-pb::clamp_depth(tlast), g.mu[m], s_imu[m])) -
                      0.5 * acc[m];
            total += val * g.weights[m];
        }
    }
    return total;
}

template <int MU, bool kTwo>
__global__ __launch_bounds__(kBlock) void k_cloudy_emission(CloudArgs a, EmissionGeom g)
{
    extern __shared__ double s_kt[];        // [2][nlayers]: kKB T of this walker and its reciprocal
    const int w = blockIdx.y;
    const int nlayers = a.nlayers, nwave = a.nwave, rtop = a.itop;
    const bool deck = a.deck_itop != nullptr;
    const bool need_clear = a.f_patchy || a.clear;
    const int dk = deck ? pb::deck_layer(a.deck_itop, w, nlayers) : -1;
    planck_terms(s_kt, g.temp + (int64_t)w * nlayers, nlayers, g.mu, g.nmu);
    if (deck) {
        if (threadIdx.x == 0)
            pb::sane_divisor(pb::kKB * uniform_f64(a.deck_surf + w), s_kt[dk], s_kt[nlayers + dk]);
        __syncthreads();
    }
    const double *s_imu = s_kt + 2 * nlayers;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nwave)
        return;
    const double *ec = a.ec + (int64_t)w * nlayers * nwave + j;
    const double *h = g.intervals + (int64_t)w * (nlayers - 1);
    const double wn = g.wn[j];
    const double factor = planck_factor(wn);
    CloudWalk cloud;
    if (kTwo)
        cloud.init(a.cl, w, j, nlayers);
    // the sums of the clear column (kTwo) or of both (one optical depth down to the deck)
    double acc[MU], eprev[MU], acc_c[kTwo ? MU : 1], eprev_c[kTwo ? MU : 1];
#pragma unroll
    for (int m = 0; m < MU; m++) {
        acc[m] = 0.0;
        eprev[m] = m < g.nmu ? pb::exp_s(pb::quot_fast(-0.0, g.mu[m], s_imu[m])) : 0.0;
        if constexpr (kTwo) {
            acc_c[m] = 0.0;
            eprev_c[m] = eprev[m];
        }
    }
    double bprev = planck_q(factor, wn, s_kt[rtop], s_kt[nlayers + rtop]);
    double depth = 0.0, depth_c = 0.0;
    double prev = ec[(int64_t)rtop * nwave];
    double prev_c = kTwo ? prev + cloud.at(rtop) : 0.0;
    const int kend = deck ? dk : nlayers - 1;                 // the cloudy column's deepest layer
    bool open_l = need_clear, open_c = true;
    double total_l = 0.0, total_c = 0.0;
    if (deck && dk <= rtop) {
        // the deck at or above the top layer: its emission, unattenuated (depth is zero there)
        total_c = emission_total<MU>(planck_q(factor, wn, s_kt[dk], s_kt[nlayers + dk]), 0.0, acc,
                                     dk, rtop, g, s_imu);
        open_c = false;
    }
    for (int k = rtop + 1; k < nlayers && (open_l || open_c); k++) {
        const double cur = ec[(int64_t)k * nwave];
        const double bnext = planck_q(factor, wn, s_kt[k], s_kt[nlayers + k]);
        const double bsum = bnext + bprev;
        if constexpr (kTwo) {
            const double cur_c = cur + cloud.at(k);
            if (open_c) {
                depth_c += 0.5 * h[k - 1] * (cur_c + prev_c);
                const double dq = pb::clamp_depth(depth_c);
#pragma unroll
                for (int m = 0; m < MU; m++) {
                    if (m < g.nmu) {
                        const double e = pb::exp_s(pb::quot_fast(-dq, g.mu[m], s_imu[m]));
                        acc_c[m] += (e - eprev_c[m]) * bsum;
                        eprev_c[m] = e;
                    }
                }
                if (depth_c >= a.maxdepth || k == kend || k == nlayers - 1) {
                    total_c = emission_total<MU>(bnext, depth_c, acc_c, k, rtop, g, s_imu);
                    open_c = false;
                }
            }
            prev_c = cur_c;
        }
        if (open_l || !kTwo) {
            depth += 0.5 * h[k - 1] * (cur + prev);
            const double dq = pb::clamp_depth(depth);         // (exp(-inf / mu) = 0 without a NaN)
#pragma unroll
            for (int m = 0; m < MU; m++) {
                if (m < g.nmu) {
                    const double e = pb::exp_s(pb::quot_fast(-dq, g.mu[m], s_imu[m]));
                    acc[m] += (e - eprev[m]) * bsum;
                    eprev[m] = e;
                }
            }
            const bool cross = depth >= a.maxdepth || k == nlayers - 1;
            if (!kTwo && open_c && (cross || k == kend)) {
                total_c = emission_total<MU>(bnext, depth, acc, k, rtop, g, s_imu);
                open_c = false;
            }
            if (open_l && cross) {
                total_l = emission_total<MU>(bnext, depth, acc, k, rtop, g, s_imu);
                open_l = false;
            }
        }
        prev = cur;
        bprev = bnext;
    }
    // (itop == nlayers - 1: no interval; the top layer's emission, as k_emission_fused)
    if (open_l || open_c) {
        double zero[MU];
#pragma unroll
        for (int m = 0; m < MU; m++)
            zero[m] = 0.0;
        const double b = planck_q(factor, wn, s_kt[rtop], s_kt[nlayers + rtop]);
        const double t = emission_total<MU>(b, 0.0, zero, rtop, rtop, g, s_imu);
        if (open_l)
            total_l = t;
        if (open_c)
            total_c = t;
    }
    cloud_store(a, w, j, total_l, total_c);
}

using pb::check_cloud;

}  // namespace

extern "C" {

int pb_deck_state_batch(int32_t *itop_d, double *rsurf_d, double *tsurf_d,
                        const double *pressure_d, const double *logp_d, const double *radius_d,
                        int64_t radius_stride, const double *temps_d, int nlayers, int nwalkers,
                        void *stream)
{
    PB_REQUIRE(nlayers >= 1 && nwalkers >= 0, "pb_deck_state_batch: bad shape");
    PB_REQUIRE(radius_stride == 0 || radius_stride >= nlayers,
               "pb_deck_state_batch: radius_stride must be 0 or at least nlayers");
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(itop_d && rsurf_d && tsurf_d && pressure_d && logp_d && radius_d && temps_d,
               "pb_deck_state_batch: null pointer");
    k_deck_state<<<pb::div_up(nwalkers, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        itop_d, rsurf_d, tsurf_d, pressure_d, logp_d, radius_d, radius_stride, temps_d, nlayers,
        nwalkers);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_cloud_plan(double *f_d, double *rows_d, const pb_cloud_models *models,
                  const double *temps_d, const double *pars_d, int pars_stride,
                  const double *wn_d, int nlayers, int nwave, int nwalkers, void *stream)
{
    PB_REQUIRE(models && models->nr >= 1 && models->nr <= kMaxCloud,
               "pb_cloud_plan: 1 ... %d cloud models", kMaxCloud);
    PB_REQUIRE(nlayers >= 1 && nwave >= 0 && nwalkers >= 0 && pars_stride >= 0,
               "pb_cloud_plan: bad shape");
    int nlec = 0;
    for (int m = 0; m < models->nr; m++) {
        PB_REQUIRE(models->kind[m] == 1 || models->kind[m] == 2,
                   "pb_cloud_plan: model %d: kind 1 (Lecavelier) or 2 (CCSgray)", m);
        PB_REQUIRE(models->pressure_d[m] && models->par[m] >= 0,
                   "pb_cloud_plan: model %d: null pressure or negative parameter index", m);
        nlec += models->kind[m] == 1;
    }
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(f_d && temps_d && pars_d && (nlec == 0 || (rows_d && wn_d)),
               "pb_cloud_plan: null pointer");
    PlanArgs a{f_d, rows_d, temps_d, pars_d, wn_d, pars_stride, nlayers, nwave, nwalkers, *models};
    hipStream_t s = pb::as_stream(stream);
    k_cloud_plan<<<pb::div_up((int64_t)nwalkers * nlayers, kBlock), kBlock, 0, s>>>(a);
    PB_LAUNCH_CHECK();
    if (nlec && nwave > 0) {
        dim3 grid(pb::div_up(nwave, kBlock), nwalkers, nlec);
        k_cloud_rows<<<grid, kBlock, 0, s>>>(a);
        PB_LAUNCH_CHECK();
    }
    return PB_OK;
}

int pb_cloudy_transit_batch(double *spectrum_d, double *clear_d, double *cloudy_d,
                            const double *ec_d, const double *raypath_d, int64_t path_stride,
                            const double *radius_d, int64_t radius_stride,
                            const int32_t *column_d, double rstar, int itop, double maxdepth,
                            int nlayers, int nwave, int nwalkers, const int32_t *deck_itop_d,
                            const double *deck_rsurf_d, const pb_cloud_terms *cloud,
                            const double *f_patchy_d, void *stream)
{
    PB_REQUIRE(nlayers >= 1 && nwave >= 0 && nwalkers >= 0, "pb_cloudy_transit_batch: bad shape");
    PB_REQUIRE(itop >= 0 && itop < nlayers, "pb_cloudy_transit_batch: itop out of range");
    const int nrow = nlayers - itop;
    const int64_t npath = ((int64_t)nrow * (nrow - 1)) / 2;
    PB_REQUIRE(nrow <= 1024, "pb_cloudy_transit_batch: at most 1024 impact parameters (got %d)",
               nrow);
    PB_REQUIRE((path_stride == 0 || path_stride >= npath) &&
               (radius_stride == 0 || radius_stride >= nlayers),
               "pb_cloudy_transit_batch: a stride must be 0 or at least a walker's length");
    PB_REQUIRE(!deck_itop_d == !deck_rsurf_d,
               "pb_cloudy_transit_batch: deck_itop_d and deck_rsurf_d go together");
    if (int rc = check_cloud(cloud, "pb_cloudy_transit_batch"))
        return rc;
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(spectrum_d && ec_d && radius_d && (raypath_d || npath == 0),
               "pb_cloudy_transit_batch: null pointer");
    CloudArgs a{spectrum_d, clear_d, cloudy_d, ec_d, column_d, deck_itop_d, deck_rsurf_d,
                f_patchy_d, maxdepth, itop, nlayers, nwave, {}};
    const bool two = cloud && cloud->nr > 0;
    if (two)
        a.cl = *cloud;
    // (no ray path at one impact parameter: the kernel then reads none)
    TransitGeom g{raypath_d ? raypath_d : radius_d, radius_d, path_stride, radius_stride, rstar};
    dim3 grid(pb::div_up(nwave, kBlock), nwalkers);
    hipStream_t s = pb::as_stream(stream);
    const bool wide = (size_t)nrow * 16 * 8 <= 48 * 1024;
    const size_t lds = (size_t)nrow * (wide ? 16 : 8) * 8;
    if (wide && two)
        k_cloudy_transit<16, true><<<grid, kBlock, lds, s>>>(a, g);
    else if (wide)
        k_cloudy_transit<16, false><<<grid, kBlock, lds, s>>>(a, g);
    else if (two)
        k_cloudy_transit<8, true><<<grid, kBlock, lds, s>>>(a, g);
    else
        k_cloudy_transit<8, false><<<grid, kBlock, lds, s>>>(a, g);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_cloudy_emission_batch(double *flux_d, double *clear_d, double *cloudy_d, const double *ec_d,
                             const double *intervals_d, const double *wn_d, const double *temp_d,
                             const double *mu_d, const double *weights_d, const int32_t *column_d,
                             int nmu, double maxdepth, int itop, int nlayers, int nwave,
                             int nwalkers, const int32_t *deck_itop_d, const double *deck_tsurf_d,
                             const pb_cloud_terms *cloud, const double *f_patchy_d, void *stream)
{
    PB_REQUIRE(nlayers >= 1 && nwave >= 0 && nwalkers >= 0, "pb_cloudy_emission_batch: bad shape");
    PB_REQUIRE(nmu >= 1 && nmu <= kMaxMu, "pb_cloudy_emission_batch: nmu must be 1..%d", kMaxMu);
    PB_REQUIRE(itop >= 0 && itop < nlayers, "pb_cloudy_emission_batch: itop out of range");
    PB_REQUIRE(!deck_itop_d == !deck_tsurf_d,
               "pb_cloudy_emission_batch: deck_itop_d and deck_tsurf_d go together");
    if (int rc = check_cloud(cloud, "pb_cloudy_emission_batch"))
        return rc;
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(flux_d && ec_d && (intervals_d || nlayers == 1) && wn_d && temp_d && mu_d &&
               weights_d, "pb_cloudy_emission_batch: null pointer");
    CloudArgs a{flux_d, clear_d, cloudy_d, ec_d, column_d, deck_itop_d, deck_tsurf_d,
                f_patchy_d, maxdepth, itop, nlayers, nwave, {}};
    const bool two = cloud && cloud->nr > 0;
    if (two)
        a.cl = *cloud;
    EmissionGeom g{intervals_d, wn_d, temp_d, mu_d, weights_d, nmu};
    dim3 grid(pb::div_up(nwave, kBlock), nwalkers);
    hipStream_t s = pb::as_stream(stream);
    const size_t lds = ((size_t)2 * nlayers + kMaxMu) * 8;
    PB_REQUIRE(lds <= 64 * 1024, "pb_cloudy_emission_batch: too many layers (%d)", nlayers);
    if (nmu <= 8 && two)
        k_cloudy_emission<8, true><<<grid, kBlock, lds, s>>>(a, g);
    else if (nmu <= 8)
        k_cloudy_emission<8, false><<<grid, kBlock, lds, s>>>(a, g);
    else if (two)
        k_cloudy_emission<kMaxMu, true><<<grid, kBlock, lds, s>>>(a, g);
    else
        k_cloudy_emission<kMaxMu, false><<<grid, kBlock, lds, s>>>(a, g);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
