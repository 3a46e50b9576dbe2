// Walker-batched retrieval path (BASELINE config 5), first stage: the cross-section table
// interpolated for a batch of atmospheres -- interp_ec (opacity/line_sampling.py:394-463 ->
// src_c/_extcoeff.c:367-418) for nw walkers in ONE launch, the walker index being a grid
// dimension, the table read once per chunk of walkers instead of once per walker:
//   k_interp_weights     per (walker, layer): the temperature bracket and the products weight x density
//   k_interp_ec_batch    ec[w][L][W] = sum_s dens[w][L][s] * lerp_T(etable[s][.][L][W]), with the
//                        continuum and alkali terms of pb_interp_cont.h added in its store
//   k_interp_ec_batch2   the same without a continuum, two adjacent samples per thread
// Which of them a call runs, in how many chunks, is plan_interp()'s decision; launch_interp()
// launches what the plan names.  The stages that follow are pb_transit.hip, pb_emission.hip,
// pb_two_stream.hip and pb_bands.hip.
#include <algorithm>
#include <cstdlib>

#include "pb_common.h"
#include "pb_interp.h"
#include "pb_interp_cont.h"

namespace {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------
// Layers nobody reads (round 5).  With the columns of a retrieval batch in the depth order of a base
// model (TableSpectrum.order_columns) the row tile at which the transit kernel leaves a column is
// known in advance to within a layer or two: tile[b] = the last ROW TILE (16 impact parameters)
// the columns 256 b ... 256 b + 255 can need (base model's deepest crossing in the block + a
// margin).  The interpolation then writes the layers row0 ... row0 + 16 (tile[b] + 1) - 1 only
// (at C5's shape 80 % of ec: 0.8 GB of 4.1 GB per 64 walkers less), and the transit kernel, should
// a walker's column still be open beyond that tile, raises flags[walker] and flags[nwalkers]
// instead of reading what was never written.  `gate` (repair pass): a launch whose workgroups
// return at once unless the flag it points to is set -- the full interpolation gated on
// flags[nwalkers], the transit of walker w gated on flags[w] -- so the repair costs two nearly
// empty launches when nothing was flagged, and no host synchronisation ever.
// ---------------------------------------------------------------------------
using pb::TileLimit;
using pb::uniform_i32;
using pb::layer_wanted;
using pbi::ContEpi;
using pbi::ContState;

// ---------------------------------------------------------------------------
// interp_ec for a batch of walkers, assigning form.  Workgroup = (256 wavenumbers, layer,
// chunk of walkers).  Walkers of a chunk that share a temperature bracket share its two table
// slices: the brackets the chunk uses at this layer are walked in ascending order, the upper
// node of one bracket staying in registers as the lower node of the next; a walker is computed
// in the pass of its own bracket.  Per-(walker, layer) brackets and weights come from
// k_interp_weights (wave-uniform loads).  kS = species held in registers (<= 8).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_interp_weights(
    int32_t *tlo_out, double *coef_out, const double *ttable, const double *temps,
    const double *density, int nmol, int ncoef, int ntemp, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const double t = temps[i];
    // same bracket rule as k_interp_ec (src_c/_extcoeff.c:394-398), clamped at the table's ends
    int tlo = pb::nearest_index(ttable, t, 0, ntemp - 1);
    if (t < ttable[tlo] || tlo == ntemp - 1)
        tlo--;
    tlo = max(tlo, 0);
    const double span = ttable[tlo + 1] - ttable[tlo];
    const double a = (ttable[tlo + 1] - t) / span, c = (t - ttable[tlo]) / span;
    tlo_out[i] = tlo;
    // the products interp_ec forms per sample, once per (walker, layer): w_lo*d_j, w_hi*d_j
    double *co = coef_out + i * 2 * ncoef;
    for (int j = 0; j < ncoef; j++) {
        const double d = j < nmol ? density[i * nmol + j] : 0.0;
        co[j] = a * d;
        co[ncoef + j] = c * d;
    }
}

// kFull: nmol == kS, no per-species predicate (the coefficient loads of a walker then merge into
// one scalar load and one wait)
template <int kS, bool kFull, int kCont = 0, bool kAlk = false>
__global__ __launch_bounds__(kBlock) void k_interp_ec_batch(
    double *ec, const double *etable, const int32_t *tlo, const double *coef, int nmol,
    int ntemp, int nlayers, int nwave, int nwalkers, int chunk, TileLimit lim, ContEpi cont = {})
{
    if (!layer_wanted(lim, blockIdx.y, blockIdx.x * kBlock, blockIdx.x * kBlock + kBlock, nwave))
        return;
    // per-(walker, layer) brackets and coefficients are wave-uniform: through the constant
    // address space they are SCALAR loads (one s_load_dwordx16 per walker at four species)
    typedef const double __attribute__((address_space(4))) *ccoef_t;
    typedef const int32_t __attribute__((address_space(4))) *ctlo_t;
    const ctlo_t ctlo = (ctlo_t)(unsigned long long)tlo;
    const int k = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int w0 = blockIdx.z * chunk, w1 = min(w0 + chunk, nwalkers);
    // brackets used by the chunk at this layer
    int bmin = ntemp, bmax = -1;
    for (int w = w0; w < w1; w++) {
        const int b = ctlo[(int64_t)w * nlayers + k];
        bmin = min(bmin, b);
        bmax = max(bmax, b);
    }
    if (i >= nwave)
        return;
    const int64_t slice = (int64_t)nlayers * nwave;
    const double *tab = etable + (int64_t)k * nwave + i;      // + (j*ntemp + t)*slice
    double lo[kS], hi[kS];
#pragma unroll
    for (int j = 0; j < kS; j++)
        hi[j] = kFull || j < nmol ? tab[((int64_t)j * ntemp + bmin) * slice] : 0.0;
    ContState<kCont, kAlk> cst;
    if constexpr (kCont != 0)
        cont_init(cst, cont, i, nwave);
    for (int b = bmin; b <= bmax; b++) {
#pragma unroll
        for (int j = 0; j < kS; j++) {
            lo[j] = hi[j];
            hi[j] = kFull || j < nmol ? tab[((int64_t)j * ntemp + b + 1) * slice] : 0.0;
        }
        // (the walkers of bracket b as the set bits of a ballot over per-lane brackets -- no
        // scalar load and wait per walker and bracket -- measured slower: 1.21 against 1.11 ms)
        for (int w = w0; w < w1; w++) {
            const int64_t wk = (int64_t)w * nlayers + k;
            if (ctlo[wk] != b)
                continue;                                   // wave-uniform
            const ccoef_t co = (ccoef_t)(unsigned long long)(coef + wk * 2 * kS);
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < kS; j++)
                if (kFull || j < nmol)
                    acc += lo[j] * co[j] + hi[j] * co[kS + j];
            if constexpr (kCont != 0)
                acc = cont_apply(acc, cst, cont, i, w, wk, nwave);
            ec[wk * nwave + i] = acc;
        }
    }
}

// Two adjacent samples per thread (16 bytes per lane and access: 1 KiB per wavefront store instead of
// 512 B).  The rows of ec and of the table start at layer * nwave samples, 8-byte aligned only when
// nwave is odd, so the pairs start at the first EVEN absolute element of the row: the accesses are
// then 16-byte aligned; the odd sample in front of / behind the pairs is done by one lane on its own.
// NP = pair slots per thread, kBlock slots apart (every store instruction of a workgroup still
// covers 4 KiB of consecutive samples): NP = 2 halves the per-walker scalar loads, waits and
// branches per byte written (0.902 against 0.914 ms per 64 walkers at C5's shape, same bits).
template <int kS, bool kFull, int NP>
__global__ __launch_bounds__(kBlock) void k_interp_ec_batch2(
    double *ec, const double *etable, const int32_t *tlo, const double *coef, int nmol,
    int ntemp, int nlayers, int nwave, int nwalkers, int chunk, TileLimit lim)
{
    // (slots [x NP kBlock, (x + 1) NP kBlock) hold the samples 2 q - 1 ... 2 q + 1)
    if (!layer_wanted(lim, blockIdx.y, 2 * (int)blockIdx.x * NP * kBlock - 1,
                      2 * ((int)blockIdx.x + 1) * NP * kBlock + 1, nwave))
        return;
    typedef const double __attribute__((address_space(4))) *ccoef_t;
    typedef const int32_t __attribute__((address_space(4))) *ctlo_t;
    typedef double d2 __attribute__((ext_vector_type(2)));
    const ctlo_t ctlo = (ctlo_t)(unsigned long long)tlo;
    const int k = blockIdx.y;
    const int w0 = blockIdx.z * chunk, w1 = min(w0 + chunk, nwalkers);
    int bmin = ntemp, bmax = -1;
    for (int w = w0; w < w1; w++) {
        const int b = ctlo[(int64_t)w * nlayers + k];
        bmin = min(bmin, b);
        bmax = max(bmax, b);
    }
    const int64_t slice = (int64_t)nlayers * nwave;
    // first sample of the row whose absolute element index is even (all slices / walkers share
    // the parity when slice and nlayers * nwave are of one parity -- checked by the launcher)
    const int head = (int)(((int64_t)k * nwave) & 1);
    // slot q of a row: its first sample alone when the row starts at an odd element, then pairs
    int ii[NP];
    bool live[NP], pair[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int q = (blockIdx.x * NP + p) * kBlock + threadIdx.x;
        ii[p] = head ? (q == 0 ? 0 : 1 + 2 * (q - 1)) : 2 * q;
        live[p] = ii[p] < nwave;
        pair[p] = live[p] && !(head && q == 0) && ii[p] + 1 < nwave;
        if (!live[p])
            ii[p] = 0;                                      // (a valid address; never stored)
    }
    if (!live[0])
        return;                                             // (slots ascend with p)
    const double *tab = etable + (int64_t)k * nwave;
    d2 lo[NP][kS], hi[NP][kS];
    auto load = [&](int p, int j, int b) -> d2 {
        const double *ptr = tab + ii[p] + ((int64_t)j * ntemp + b) * slice;
        if (pair[p])
            return *reinterpret_cast<const d2 *>(ptr);
        d2 v;
        v.x = ptr[0];
        v.y = 0.0;
        return v;
    };
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int j = 0; j < kS; j++)
            hi[p][j] = kFull || j < nmol ? load(p, j, bmin) : d2{0.0, 0.0};
    for (int b = bmin; b <= bmax; b++) {
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int j = 0; j < kS; j++) {
                lo[p][j] = hi[p][j];
                hi[p][j] = kFull || j < nmol ? load(p, j, b + 1) : d2{0.0, 0.0};
            }
        for (int w = w0; w < w1; w++) {
            const int64_t wk = (int64_t)w * nlayers + k;
            if (ctlo[wk] != b)
                continue;                                   // wave-uniform
            const ccoef_t co = (ccoef_t)(unsigned long long)(coef + wk * 2 * kS);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                d2 acc = {0.0, 0.0};
#pragma unroll
                for (int j = 0; j < kS; j++)
                    if (kFull || j < nmol) {
                        // same products and sums per sample as the one-sample kernel
                        acc.x += lo[p][j].x * co[j] + hi[p][j].x * co[kS + j];
                        acc.y += lo[p][j].y * co[j] + hi[p][j].y * co[kS + j];
                    }
                double *dst = ec + wk * nwave + ii[p];
                if (pair[p])
                    *reinterpret_cast<d2 *>(dst) = acc;
                else if (live[p])
                    dst[0] = acc.x;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// one interpolation launch: environment, plan, then the kernel of the planned form
// ---------------------------------------------------------------------------

// The PB_INTERP_* variables a launch consults.  Read at the top of EVERY launch, never kept in a
// static: the tests change them between calls of one process.
struct InterpTuning {
    int chunk = 64;                // PB_INTERP_CHUNK: walkers per chunk before the workgroup rule
    bool pairs = true;             // PB_INTERP_PAIRS=0: one sample per thread
    int np = 0;                    // PB_INTERP_NP as 2 or 1 (any other value); 0 = not set
    bool full = true;              // PB_INTERP_FULL=0: four species run the predicated instantiation
};

InterpTuning read_interp_tuning()
{
    InterpTuning t;
    if (const char *e = getenv("PB_INTERP_CHUNK"))
        t.chunk = std::max(1, atoi(e));
    if (const char *e = getenv("PB_INTERP_PAIRS"))
        t.pairs = atoi(e) != 0;
    if (const char *e = getenv("PB_INTERP_NP"))
        t.np = atoi(e) == 2 ? 2 : 1;
    if (const char *e = getenv("PB_INTERP_FULL"))
        t.full = atoi(e) != 0;
    return t;
}

// what plan_interp() decides from
struct InterpShape {
    int nmol, nlayers, nwave, nwalkers;
    bool aligned16;                // ec_d and etable_d both on 16 bytes
    int kcont;                     // the continuum's form (pbi::ContLaunch)
    bool kalk;
};

// What a launch will run, decided from the shape and the environment alone.
struct InterpPlan {
    int chunk;                     // walkers per workgroup
    bool pairs;                    // k_interp_ec_batch2 (only without a continuum)
    int np;                        // its pair slots per thread
    int kS;                        // species held in registers
    bool kFull;
    int kcont;
    bool kalk;
    dim3 grid;
};

InterpPlan plan_interp(const InterpShape &c, const InterpTuning &tn)
{
    InterpPlan p;
    // walkers per chunk: every chunk reads the table slices its walkers bracket again, so as many
    // as the launch can afford while it still fills the chip (C5, 64 walkers: 1.40 ms in chunks
    // of 16, 1.23 in one chunk, 1.11 with the species count a template constant)
    p.chunk = tn.chunk;
    while (p.chunk > 1 && (int64_t)pb::div_up(c.nwave, kBlock) * c.nlayers *
                                  pb::div_up(c.nwalkers, p.chunk) < 2048)
        p.chunk /= 2;
    p.grid = dim3(pb::div_up(c.nwave, kBlock), c.nlayers, pb::div_up(c.nwalkers, p.chunk));
    // two samples per thread when every row of every slice / walker has the parity of its layer
    // index times nwave (slice = nlayers * nwave even, or nwave even), and 16-byte aligned bases
    p.pairs = tn.pairs && c.nwave >= 4 && (((int64_t)c.nlayers * c.nwave) % 2 == 0) && c.aligned16;
    // two pair slots per thread for launches that still fill the chip with half the workgroups
    // (up to four species: with eight, 146 registers would cost a wavefront per SIMD)
    p.np = 1;
    if (p.pairs && c.nmol <= 4 && (int64_t)pb::div_up(c.nwave / 2 + 2, 2 * kBlock) * c.nlayers *
                                          pb::div_up(c.nwalkers, p.chunk) >= 4096)
        p.np = 2;
    if (tn.np)
        p.np = tn.np;
    // with a continuum: one sample per thread.  The pair kernel with the epilogue needs 181 / 234
    // VGPRs (continuum / + H-: two wavefronts per SIMD) and ran slower at C5's shape: 1.48 against
    // 1.10 ms mean per launch, 4.35 against 3.69 ms per 64-walker transit step
    p.kcont = c.kcont;
    p.kalk = c.kalk;
    if (p.pairs && !p.kcont)
        p.grid.x = pb::div_up(c.nwave / 2 + 2, kBlock * p.np);
    p.kS = pbi::interp_ncoef(c.nmol);
    p.kFull = c.nmol == 8 || (c.nmol == 4 && tn.full);
    return p;
}

// the arguments every form takes
struct InterpCall {
    double *ec;
    const double *etable;
    const int32_t *tlo;
    const double *coef;
    int nmol, ntemp, nlayers, nwave, nwalkers;
    TileLimit lim;
};

template <typename... Epi>
void run_interp(void (*kernel)(double *, const double *, const int32_t *, const double *, int, int,
                               int, int, int, int, TileLimit, Epi...),
                const InterpPlan &p, const InterpCall &c, hipStream_t s, const Epi &...epi)
{
    kernel<<<p.grid, kBlock, 0, s>>>(c.ec, c.etable, c.tlo, c.coef, c.nmol, c.ntemp, c.nlayers,
                                     c.nwave, c.nwalkers, p.chunk, c.lim, epi...);
}

template <int kS, bool kFull, int kCont>
void launch_interp_cont(const InterpPlan &p, const InterpCall &c, const ContEpi &epi, hipStream_t s)
{
    if (p.kalk)
        run_interp(k_interp_ec_batch<kS, kFull, kCont, true>, p, c, s, epi);
    else
        run_interp(k_interp_ec_batch<kS, kFull, kCont, false>, p, c, s, epi);
}

template <int kS, bool kFull>
void launch_interp_form(const InterpPlan &p, const InterpCall &c, const ContEpi &epi, hipStream_t s)
{
    if (p.kcont == 1)
        launch_interp_cont<kS, kFull, 1>(p, c, epi, s);
    else if (p.kcont == 2)
        launch_interp_cont<kS, kFull, 2>(p, c, epi, s);
    else if (p.pairs && p.np == 2)
        run_interp(k_interp_ec_batch2<kS, kFull, 2>, p, c, s);
    else if (p.pairs)
        run_interp(k_interp_ec_batch2<kS, kFull, 1>, p, c, s);
    else
        run_interp(k_interp_ec_batch<kS, kFull, 0, false>, p, c, s, ContEpi{});
}

int launch_interp(const InterpPlan &p, const InterpCall &c, const ContEpi &epi, hipStream_t s)
{
    if (p.kS == 4 && p.kFull)
        launch_interp_form<4, true>(p, c, epi, s);
    else if (p.kS == 4)
        launch_interp_form<4, false>(p, c, epi, s);
    else if (p.kFull)
        launch_interp_form<8, true>(p, c, epi, s);
    else
        launch_interp_form<8, false>(p, c, epi, s);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

// check the call, lay out the workspace, write the weights and prepare the continuum (a gated
// repair pass runs on what its first pass left in the workspace: same walkers, same weights, same
// records), plan, launch
int interp_ec_batch_launch(double *ec_d, const double *etable_d, const double *ttable_d,
                           const double *temps_d, const double *density_d, void *work_d, int nmol,
                           int ntemp, int nlayers, int nwave, int nwalkers, TileLimit lim,
                           void *stream, const pb_cont_batch *cont = nullptr)
{
    PB_REQUIRE(nmol >= 1 && nmol <= 8 && ntemp >= 2 && nlayers >= 1 && nwave >= 0 &&
                   nwalkers >= 0,
               "pb_interp_ec_batch: bad shape (1-8 species, >= 2 table temperatures)");
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(ec_d && etable_d && ttable_d && temps_d && density_d && work_d,
               "pb_interp_ec_batch: null pointer");
    hipStream_t s = pb::as_stream(stream);
    const int64_t n = (int64_t)nwalkers * nlayers;
    const pbi::InterpWork work =
        pbi::interp_work(work_d, n, pbi::interp_ncoef(nmol), cont ? pbi::cont_nrec(cont) : 0);
    if (!lim.gate) {
        const int rc = pbi::launch_interp_weights(work.coef, ttable_d, temps_d, density_d, nmol,
                                                  ntemp, n, s);
        if (rc != PB_OK)
            return rc;
    }
    pbi::ContLaunch cl;
    if (cont) {
        const int rc = pbi::cont_prepare(&cl, cont, work, temps_d, nlayers, nwave, nwalkers,
                                         lim.gate != nullptr, s);
        if (rc != PB_OK)
            return rc;
    }
    const bool aligned16 = (uintptr_t)ec_d % 16 == 0 && (uintptr_t)etable_d % 16 == 0;
    const InterpPlan p = plan_interp({nmol, nlayers, nwave, nwalkers, aligned16, cl.kcont, cl.kalk},
                                     read_interp_tuning());
    return launch_interp(p, {ec_d, etable_d, work.tlo, work.coef, nmol, ntemp, nlayers, nwave,
                             nwalkers, lim}, cl.epi, s);
}

}  // namespace

namespace pbi {

int launch_interp_weights(double *coef, const double *ttable_d, const double *temps_d,
                          const double *density_d, int nmol, int ntemp, int64_t n, hipStream_t s)
{
    const int ncoef = interp_ncoef(nmol);
    k_interp_weights<<<pb::div_up(n, kBlock), kBlock, 0, s>>>(interp_tlo(coef, n, ncoef), coef,
                                                            ttable_d, temps_d, density_d, nmol,
                                                            ncoef, ntemp, n);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace pbi

extern "C" {

int64_t pb_interp_ec_batch_work_doubles(int nlayers, int nwalkers)
{
    if (nlayers < 0 || nwalkers < 0)
        return -1;
    return pbi::interp_work_doubles((int64_t)nwalkers * nlayers);
}

int pb_interp_ec_batch_plan(int32_t *out, int nmol, int nlayers, int nwave, int nwalkers,
                            int aligned16, int kcont, int kalk)
{
    PB_REQUIRE(out && nmol >= 1 && nmol <= 8 && nlayers >= 1 && nwave >= 1 && nwalkers >= 1 &&
                   kcont >= 0 && kcont <= 2,
               "pb_interp_ec_batch_plan: bad shape (1-8 species, continuum form 0-2)");
    const InterpPlan p = plan_interp({nmol, nlayers, nwave, nwalkers, aligned16 != 0, kcont,
                                      kalk != 0}, read_interp_tuning());
    const int32_t v[6] = {p.chunk, p.pairs, p.np, p.kS, p.kFull, (int32_t)p.grid.x};
    std::copy(v, v + 6, out);
    return PB_OK;
}

int pb_interp_ec_batch(double *ec_d, const double *etable_d, const double *ttable_d,
                       const double *temps_d, const double *density_d, void *work_d, int nmol,
                       int ntemp, int nlayers, int nwave, int nwalkers, void *stream)
{
    return interp_ec_batch_launch(ec_d, etable_d, ttable_d, temps_d, density_d, work_d, nmol, ntemp,
                                  nlayers, nwave, nwalkers, TileLimit{nullptr, 0, nullptr}, stream);
}

int pb_interp_ec_batch_limited(double *ec_d, const double *etable_d, const double *ttable_d,
                               const double *temps_d, const double *density_d, void *work_d,
                               int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                               const int32_t *tile_limit_d, int row0, const int32_t *gate_d,
                               void *stream)
{
    PB_REQUIRE(row0 >= 0 && row0 < std::max(nlayers, 1), "pb_interp_ec_batch_limited: row0 out of range");
    return interp_ec_batch_launch(ec_d, etable_d, ttable_d, temps_d, density_d, work_d, nmol, ntemp,
                                  nlayers, nwave, nwalkers, TileLimit{tile_limit_d, row0, gate_d},
                                  stream);
}

int64_t pb_interp_ec_batch_cont_work_doubles(const pb_cont_batch *cont, int nlayers, int nwave,
                                             int nwalkers)
{
    const int nrec = pbi::cont_nrec(cont);
    if (nrec < 0 || nlayers < 0 || nwave < 0 || nwalkers < 0)
        return -1;
    return pbi::interp_work_doubles((int64_t)nwalkers * nlayers, nrec, pbi::cont_nlec(cont),
                                    nwalkers, nwave);
}

int pb_interp_ec_batch_cont(double *ec_d, const double *etable_d, const double *ttable_d,
                            const double *temps_d, const double *density_d, void *work_d,
                            int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                            const pb_cont_batch *cont, void *stream)
{
    const int rc = pbi::cont_check(cont);
    if (rc != PB_OK)
        return rc;
    return interp_ec_batch_launch(ec_d, etable_d, ttable_d, temps_d, density_d, work_d, nmol, ntemp,
                                  nlayers, nwave, nwalkers, TileLimit{nullptr, 0, nullptr}, stream,
                                  cont);
}

int pb_interp_ec_batch_cont_limited(double *ec_d, const double *etable_d, const double *ttable_d,
                                    const double *temps_d, const double *density_d, void *work_d,
                                    int nmol, int ntemp, int nlayers, int nwave, int nwalkers,
                                    const pb_cont_batch *cont, const int32_t *tile_limit_d,
                                    int row0, const int32_t *gate_d, void *stream)
{
    const int rc = pbi::cont_check(cont);
    if (rc != PB_OK)
        return rc;
    PB_REQUIRE(row0 >= 0 && row0 < std::max(nlayers, 1),
               "pb_interp_ec_batch_cont_limited: row0 out of range");
    return interp_ec_batch_launch(ec_d, etable_d, ttable_d, temps_d, density_d, work_d, nmol, ntemp,
                                  nlayers, nwave, nwalkers, TileLimit{tile_limit_d, row0, gate_d},
                                  stream, cont);
}

}  // extern "C"
