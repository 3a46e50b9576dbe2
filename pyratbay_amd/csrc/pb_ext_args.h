// Argument block, record formats, kernel geometry and __device__ helpers shared by the translation
// units of the line-by-line extinction: pb_extinction.hip (handle, planner, C ABI),
// pb_ext_records.hip (layer state and records), pb_ext_gather.hip (the gathers of constant-step
// grids), pb_ext_resolution.hip (`resolution` plans) and, in the experiments build, pb_rounds.hip /
// pb_wave.hip.  The host side of the same units is in pb_ext_plan.h.
#pragma once

#include <cstdint>

#include "pb_common.h"
#include "pb_internal.h"

namespace pbx {

// `make EXPERIMENTS=1` (libpbhip_exp.so) keeps the measured dead ends selectable: gather modes 4
// (scatter), 5 (rounds: pb_rounds.hip) and 7 (wave: pb_wave.hip), the predicted run plans of the
// `resolution` mode.  The default library compiles none of them.
#ifdef PB_EXPERIMENTS
constexpr bool kExp = true;
#else
constexpr bool kExp = false;
#endif

// global gather (k_ext_resample): threads of a workgroup and the samples a wavefront / workgroup owns
constexpr int kBlock = 256;
constexpr int kChunks = 2;                       // 128-sample chunks per wavefront
constexpr int kLaneSamples = 2;                  // consecutive samples per lane (16-B loads)
constexpr int kChunk = 64 * kLaneSamples;        // samples per chunk
constexpr int kWaveSpan = kChunks * kChunk;      // samples per wavefront
constexpr int kTile = 4 * kWaveSpan;             // output samples per workgroup
constexpr int kRecs = 4;                         // records in flight per wavefront trip
static_assert(kTile <= kPmPad, "table padding must cover one tile");
static_assert(kTile < 65536, "window coordinates are packed in 16 bits");

// packed records (k_records writes them; the staged gather and the planner decode them)
constexpr int kLongLenBits = 14;   // window length in a long-row record (rows of up to 16 x 1024 samples)
constexpr int kChunkRow = 1024;      // samples per chunk of a long phase row (= kStageRowMax)
constexpr int kRecLayers = 8;        // layers per thread of k_records (group data loaded once, the
                                     // sample index and the Doppler column carried from layer to
                                     // layer; 4 / 8 / 10 / 16: 96 / 86 / 87 / 95 us at C2);
                                     // PB_REC_LAYERS=1: one

constexpr int kBinSamples = 256;     // output samples per bin of the phase-list position index
constexpr int kStagePad = 256;       // zero samples on either side of a staged row
constexpr int kStageSpan = 256;      // samples per wavefront and sub-tile (4 chunks of 64)
constexpr int kStageRowMax = 1024;   // longest phase row the staged kernels keep in one piece
constexpr int kStageRowsMax = 2;     // most rows (segments) one barrier step of k_ext_staged stages
constexpr int kStageRowsDefault = kStageRowsMax;   // the cap of a call that PB_STAGE_ROWS does not set

// Rows per barrier step of the staged gather (LDS-DMA path) and the pitch of their slots.  The
// row area of a workgroup is sized for two rows of `rowlds` samples, [pad][row][pad][row][pad]
// with pads of kStagePad samples; the rows of a (layer, isotope) are at most `rowlim` samples
// long, and where four or more slots of pitch rowlim + kStagePad (rounded down to even) fit the
// same area a step stages `rows` consecutive segments instead of one: slots [0, rows) on even
// steps, [rows, 2 rows) on odd ones, the pad after a slot being the pad before the next.
// The pad that is needed: a visit reads the 256 positions of a span of which at least one holds
// row data, so it reaches at most 255 positions beyond either end of the data, which lies in
// [0, rowlim) of its slot -- slots may follow each other at rowlim + 255, the next even number
// for an odd rowlim (slots start 16-byte aligned).  A piece of a row's DMA writes zeros up to 127
// samples past rowlim: inside the pad for every pitch.
// rows == 1 keeps the pitch of two full rows (rowlds is even where the planner sets it; an odd
// one is rounded down like the others, whatever the caller passes).
struct StageSlots {
    int pitch, rows;
};
__host__ __device__ inline StageSlots stage_slots(int rowlds, int rowlim, int cap = kStageRowsMax)
{
    const int area = 2 * (rowlds + kStagePad);
    const int pitch = (rowlim + kStagePad) & ~1;
    int rows = area / pitch / 2;
    if (rows > cap)
        rows = cap;
    if (rows > kStageRowsMax)
        rows = kStageRowsMax;
    if (rows < 2)
        return {(rowlds + kStagePad) & ~1, 1};
    return {pitch, rows};
}

// The slot rule: live segment g of a batch (numbered from 0 in every batch) is walked in step
// g / rows and lies in slot (g / rows & 1) * rows + g % rows -- this many BYTES after slot 0,
// with pitch8 = 8 * pitch.  rows = 1, pitch = rowlds + kStagePad: the two buffers of the one-row
// loop.  The requests of k_ext_staged place a row there (by offsets they carry from step to
// step), and on the LDS-DMA path the batch set-up adds it to the row offset of every record of the
// segment, so the walk of every segment reads from slot 0's address.
static_assert(kStageRowsMax == 2, "stage_slot_off8(): rows is a power of two");
__host__ __device__ inline unsigned stage_slot_off8(int g, int rows, unsigned pitch8)
{
    // for a power of two, (g / rows & 1) * rows + g % rows = g mod 2 rows
    return (unsigned)(g & (2 * rows - 1)) * pitch8;
}

// staged gather (k_ext_staged): wavefronts and threads of a workgroup
constexpr int kStagedWaves = 8;
constexpr int kStagedThreads = kStagedWaves * 64;
constexpr int64_t kStagedSub = kStagedWaves * kStageSpan;      // samples of one sub-tile

// resident-profile gather (k_ext_resident)
constexpr int kResWaves = 8;
constexpr int kResThreads = kResWaves * 64;
constexpr int kResStrips = 2;                              // 64-sample strips per wavefront
constexpr int kResTile = kResThreads * kResStrips;         // output samples per workgroup
constexpr int kResCapDefault = 8192;                       // doubles of LDS for one profile block
static_assert(kResTile < 65536, "window coordinates are packed in 16 bits");

// wave-autonomous gather (pb_wave.hip): output samples per workgroup (every wavefront keeps all
// of them) and the longest phase row / window it stages (three LDS-DMA pieces of 128 samples)
constexpr int kWvTile = 2048;
constexpr int kWvRowMax = 384;

struct VRec;
struct VSeg;
struct UnitHdr;

// Record of the scatter kernel: everything one wavefront needs about a (layer, group) pair,
// read with ONE scalar load.
struct __attribute__((aligned(32))) Rec32 {
    double k;            // co-added strength (before threshold / density)
    long long off;       // table element read by output sample 0 (row start + q)
    int ulo, uhi;        // window on the global output grid
    int pad[2];
};

// Record of the staged kernel: 16 bytes per (layer, phase-sorted group).  The window end, the
// row offset q and the phase follow from ulo, len, the cell's half-width and the group's
// fine index (ph_iown), so they are not stored.
struct __attribute__((aligned(16))) Rec16 {
    double k;            // co-added strength (before threshold / density)
    int32_t ulo;         // window start on the global output grid
    uint32_t lc;         // window length (12 bits) | table cell << 12
};

struct LblArgs {
    // Voigt table
    const double *pm;
    const double *flat;
    const int64_t *pm_base;
    const int32_t *pm_stride;
    const int32_t *psize;
    const int32_t *pindex;
    const double *doppler;
    const double *lorentz;
    int ndop, nlor, osamp;
    // lines and groups
    const double *lwn, *elow, *gf;
    const int32_t *lid;
    const int32_t *gfirst, *gcount, *giown;
    const int64_t *iso_gstart;
    // the same groups sorted by (isotope, iown mod osamp, iown) for the staged kernel
    const int32_t *ph_first, *ph_count, *ph_iown;
    const int64_t *ph_start;          // [niso*(osamp+1)+1]
    // coarse position index of the phase-sorted list: ph_bin[(iso*osamp + p)*(nbins+1) + b] =
    // first entry of (iso, p) at or after fine position b * kBinSamples * osamp
    const int32_t *ph_bin;
    int ph_nbins;
    int rowcap;                       // longest phase row of the table (samples)
    int rowlds;                       // longest row (or row chunk) a staged LDS buffer holds
    int rows_cap;                     // most rows per barrier step (stage_slots()); 1 = one everywhere
    const int32_t *ph_iso;            // isotope of every phase-sorted group
    const int32_t *giso;              // isotope of every position-sorted group
    // group list that k_records walks (phase-sorted or position-sorted) and whether the
    // gather kernel reads records (1) or derives them itself (0: resolution mode)
    const int32_t *rk_first, *rk_count, *rk_iown, *rk_iso;
    const double *rk_lwn, *rk_elow, *rk_gf;   // the leader line of every group, same order
    const double *g_lead;             // leader lines in position order [3][ngroups]
    int use_records;
    int64_t ngroups;
    // fine-index window of the groups whose records this call needs (a shard +- the largest
    // reach), and whether groups outside it are left out of the per-row maxima too
    int64_t rec_flo, rec_fhi;
    int kmax_local;
    // two-phase shard calls (kmax_local): the groups within [rec_flo, rec_fhi] are runs of the
    // group order k_records walks (one per (isotope, phase) in phase order, one per isotope in
    // position order); thread t of the launch takes group wm_lo[r] + t - wm_off[r] of the run r
    // that holds t, and the launch has wm_total threads per layer block instead of ngroups.
    // Index 0: the order of the phase-walking pass, 1: position order.  Null: every group.
    const int32_t *wm_lo[2];
    const int32_t *wm_off[2];
    int wm_n[2];
    int wm_lds;                       // the offsets of map 0 are copied to LDS (else bisected in global memory)
    int64_t wm_total[2];
    // resident-profile kernel: which layers it computes, its LDS capacity (doubles, 0 = off)
    // and, per isotope, the first position-sorted group at or after every output sample
    int32_t *ls_resident;
    int32_t *ls_block;                // largest phase-major profile block of the layer (doubles)
    int res_cap;
    // wave-autonomous kernel (pb_wave.hip): layers whose longest phase row is at most wave_cap
    // samples are its (ls_wave, decided by k_layer_state; 0 = kernel off) and skipped by the staged one
    int32_t *ls_wave;
    int wave_cap;
    const int32_t *gs_start;          // [niso][nwave+1]
    // scatter kernel: one 32-byte record per (layer, position-sorted group)
    struct Rec32 *rec32;
    // staged kernel: packed records of the layers it computes (null: SoA records)
    Rec16 *rec16;
    // long phase rows (> kStageRowMax samples) are cut into nch_max chunks of kStageRowMax
    // samples; every (group, chunk) then has its own packed record and the gather kernel
    // treats (phase, chunk) as a phase of its own.  Layout of a layer's records:
    // [phase p][chunk k][position] = ps*nch_max + k*cnt_p + (g - ps).  1 = no chunking.
    int nch_max;
    // line lists whose packed records exceed the plan's record budget are walked in CHUNKS of
    // consecutive (isotope, phase) keys of the phase-sorted group list: k_records and the staged
    // gather then see the groups [grp_lo, grp_hi) only (records at rec16[layer*rec_pitch + g -
    // grp_lo]), the gather walks the keys iso*osamp + phase in [key_lo, key_hi) and, from the
    // second chunk on (accumulate), continues the running sums it finds in ext -- the same terms
    // in the same order as one launch over every key.  Unchunked: grp = [0, ngroups),
    // rec_pitch = ngroups, key = [0, niso*osamp), accumulate = 0.
    int64_t grp_lo, grp_hi, rec_pitch;
    int key_lo, key_hi, accumulate;
    // staged kernel, small launches: the phases of a tile are split between nsplit workgroups
    // (see the kernel's block decoding); split 0 writes ext, the others part[split-1][layer][row][sample]
    int nsplit;
    double *part;
    // per-layer phase split of the staged kernel (null: every layer is split nsplit ways): the
    // (layer, split) units of the launch in dispatch order, unit_tab[u] = layer << 8 | split, and
    // the number of pieces of every layer; nsplit is then the largest of them (plane count)
    const int32_t *unit_tab;
    const int32_t *lsplit;
    int nunits;
    // per-tile phase split of the staged kernel (null: off): tile t of every layer is computed by
    // tsplit[t] <= nsplit workgroups; the (tile, split) workgroups beyond it end at once.  For line
    // lists of uneven density (band heads): the tiles under a head hold 10-100 x the records of
    // the others and would end the launch alone.
    const int32_t *tsplit;
    // layers a launch leaves alone (lskip[layer] != 0): the direct gather of a host-free
    // `resolution` call computes only the layers its predicted run plan did not fit
    const int32_t *lskip;
    // tsplit[t] == 0: the tile is too sparse for the staged kernel (a few records per phase row:
    // its time is its ~300 barrier steps whatever they hold) and is computed by the global gather,
    // launched beside it over the tiles so marked; ts_tile = samples per tile of that table;
    // pos2ph[g] = index of position-sorted group g in the phase-sorted list (the packed records'
    // order), for the global gather's record fetch
    int ts_tile;
    const int32_t *pos2ph;
    // per (layer, phase-sorted group) records written by k_records [nlayers][ngroups]
    double *rec_k;                    // co-added strength (before threshold / density)
    int32_t *rec_ulo, *rec_uhi;       // window on the global output grid
    int32_t *rec_q;                   // row index = output sample + q
    int32_t *rec_cell, *rec_phi;      // table cell and phase row
    double inv_osamp;
    int64_t nlines;
    // static species data
    const double *molrad, *molmass;
    const int32_t *isoimol, *isoiext;
    const double *isomass, *isoratio;
    const int32_t *divisors;
    int nmol, niso, ndivs;
    // per-call inputs
    const double *temp, *dens, *isoz;
    int64_t z_iso_stride, z_layer_stride;
    // layer state (workspace)
    int32_t *ls_ofactor, *ls_scale;
    int64_t *ls_dnwn;
    double *ls_dwnstep;
    double *ls_cutsteps, *ls_inv_ofactor, *ls_inv_scale;   // per-layer quotients for k_records
    double *ls_inv_temp;              // 1 / temperature of the layer
    double *li_invz;                  // 1 / partition function of the (layer, isotope)
    double *li_alphad, *li_dens, *li_z;
    int32_t *li_ilor, *li_hmax;
    int32_t *li_rowmax;               // longest phase row the (layer, isotope) can select
    int32_t *li_hlo, *li_hhi;         // smallest / largest profile half-width it can select
    unsigned long long *kmax_bits;
    // grid
    const double *wn;
    double own0, own_last, ownstep, wnstep, wn0;
    int64_t onwn;
    double cutoff, ethresh;
    int add, nrows, nlayers, nwave;
    int64_t wbegin, wcount;
    int ntiles;
    int experiment;      // diagnostics only (PB_EXPERIMENT): 1 = every record reads one slice
    // cycle account of the staged kernel (experiments build, PB_STAGE_PROBE=4): s_memtime ticks per
    // category and layer, probe[layer * 24 + category] (see k_ext_staged); null otherwise
    unsigned long long *probe;
    double *ext;
    // round-staged gather (pb_rounds.hip): tile and LDS row buffer (samples), the largest
    // distance (fine samples) from which a group can reach a tile, per-unit capacity offsets
    // of the visit-record / segment lists [ntiles*nsplit + 1] and the lists themselves
    int rtile, rbuf;
    int64_t reachmax;
    const int64_t *unit_cap;
    VRec *vrec;
    VSeg *vseg;
    int32_t *vrnd;     // first visit record of every round (+ one past the last)
    UnitHdr *uhdr;
    // k_records: 1 / ls_dwnstep of every layer (trunc_quot_inv)
    double *ls_inv_dwnstep;
};

size_t rounds_prep_lds(const LblArgs &a);
void rounds_geometry(int geom, int *tile, int *rbuf);
int rounds_launch(const LblArgs &a, int geom, hipStream_t s);
size_t wave_lds(const LblArgs &a);
int wave_launch(LblArgs a, int nunits, hipStream_t s);


// first index in [lo,hi) with a[idx] >= v
__device__ inline int64_t lower_bound_i32(const int32_t *a, int64_t lo, int64_t hi, int64_t v)
{
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (a[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// two lower bounds in lock step: the loads of the two bisections are independent, so every trip
// has both in flight (the candidate search of the staged gather is a chain of dependent global
// loads: its two bounds one after the other were 21 % of a rank-size launch's slot-time)
__device__ inline void lower_bound2_i32(const int32_t *a, int64_t lo0, int64_t hi0, int64_t v0,
                                        int64_t lo1, int64_t hi1, int64_t v1, int64_t &r0,
                                        int64_t &r1)
{
    while (lo0 < hi0 || lo1 < hi1) {
        const bool go0 = lo0 < hi0, go1 = lo1 < hi1;
        const int64_t mid0 = go0 ? (lo0 + hi0) >> 1 : lo0 - (lo0 > 0);
        const int64_t mid1 = go1 ? (lo1 + hi1) >> 1 : mid0;
        const int32_t x0 = a[mid0], x1 = a[mid1];
        if (go0) {
            if (x0 < v0)
                lo0 = mid0 + 1;
            else
                hi0 = mid0;
        }
        if (go1) {
            if (x1 < v1)
                lo1 = mid1 + 1;
            else
                hi1 = mid1;
        }
    }
    r0 = lo0;
    r1 = lo1;
}

// floor(a / d) for |a| < 2^31 and 0 < d < 2^20, with inv = 1.0/d: (a + 0.5)/d is never an
// integer, so the product cannot round across one.
__device__ inline int floor_div_inv(int a, double inv)
{
    return (int)floor(((double)a + 0.5) * inv);
}

// Line strength divided by the abundance (_extcoeff.c:219-224), same operation order; the three
// divisions by per-layer values through pb::quot(), the exponentials through pb::exp_s (the device
// library's exp arithmetic with its coefficients in scalar registers: same bits).  k_records
// evaluates this once per (layer, line): 2 exp + 3 divisions were 0.11 ms of every C2 spectrum.
__device__ inline double line_strength(double ratio, double gf, double elow, double wavn,
                                       double temp, double inv_temp, double z, double inv_z)
{
    const double k = pb::quot_fast(pb::kSigCte * ratio * gf *
                                       pb::exp_s(pb::quot_fast(-pb::kExpCte * elow, temp, inv_temp)) *
                                       (1 - pb::exp_s(pb::quot_fast(-pb::kExpCte * wavn, temp, inv_temp))),
                                   z, inv_z);
    // one test of the END result instead of one per quotient: a special value in any of the three
    // (temp or z zero / infinite, an infinite numerator) ends as NaN or 0 here -- then, and when
    // the strength has really underflowed, the reference's own divisions decide
    if (__builtin_expect(!(fabs(k) > 0.0), 0))
        return pb::kSigCte * ratio * gf * pb::exp_s(-pb::kExpCte * elow / temp) *
               (1 - pb::exp_s(-pb::kExpCte * wavn / temp)) / z;
    return k;
}

// a wave-uniform int written by an earlier kernel, by a scalar load
__device__ __forceinline__ int uniform_load_i32(const int32_t *p, int64_t i)
{
    typedef const int32_t __attribute__((address_space(4))) *cptr;
    return ((cptr)(unsigned long long)p)[i];
}

// A wave-uniform element of a device array written by an EARLIER kernel: read through the constant
// address space, i.e. by a scalar load (a plain load of a uniform address is a vector load that
// every lane waits for).
template <class T>
__device__ __forceinline__ T uniform_load(const T *p, int64_t i)
{
    typedef const T __attribute__((address_space(4))) *cptr;
    return ((cptr)(unsigned long long)p)[i];
}

// ---------------------------------------------------------------------------
// helpers for the gather kernels
// ---------------------------------------------------------------------------
__device__ inline double bcast(double v, int lane)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
// Window of one group on the dynamic grid, exactly as _extcoeff.c:274-299.
struct Window {
    long minj, maxj;
    int half, cell;
};

// a / d truncated toward zero like C's integer division, for |a| < 2^31, 0 < d < 2^20, inv = 1.0/d
__device__ inline int trunc_div_inv(int a, double inv)
{
    return a >= 0 ? floor_div_inv(a, inv) : -floor_div_inv(-a, inv);
}

// (int)(x / d) without the division, for a divisor whose reciprocal inv = RN(1 / d) a layer
// prepares once (k_layer_state: ls_inv_dwnstep).  q = RN(x * inv) carries two roundings,
// |q - x / d| <= |x / d| (2^-52 + 2^-106), and RN(x / d) one more of 2^-53: for |x / d| < 2^31 (the
// result is an int) q and RN(x / d) are less than 2^31 (2^-52 + 2^-53 + 2^-106) < 2^-19 apart.  So
// when q is farther than 2^-19 from every integer, both lie strictly between the same two
// consecutive integers and truncate to the same one.  Otherwise -- a line on a sample of the
// layer's grid to within 2^-19 of a step, x = 0, a quotient beyond the int range (q - (int)q is
// then 1 or more), a NaN -- the division itself decides: one test of the result, like
// line_strength's.  tests/test_records_quotient_cpu.py restates this against the division.
__device__ __forceinline__ int trunc_quot_inv(double x, double d, double inv)
{
    const double q = x * inv;
    const int t = (int)q;
    const double f = fabs(q - (double)t);
    if (__builtin_expect(!(fabs(f - 0.5) < 0.5 - 0x1p-19), 0))
        return (int)(x / d);
    return t;
}

// trunc_div_inv() without its select: a select between two calls is compiled to two predicated
// blocks, and a wavefront issues both whatever its lanes hold
__device__ __forceinline__ int trunc_div_inv_abs(int a, double inv)
{
    const int q = floor_div_inv(abs(a), inv);
    return a < 0 ? -q : q;
}

// Index of the element of the sorted a[0..n-1] closest to v, as pb::nearest_index(a, v, 0, n - 1)
// finds it, from the answer `prev` of a neighbouring search (< 0: none).  The bisection ends on
// the one pair lo, lo + 1 with a[lo] <= v < a[lo + 1] whatever range it started from, as long as
// the range holds such a pair; [prev - 1, prev + 1] does when a[prev - 1] <= v < a[prev + 1], and
// the middle element says which half.  Everything else -- no neighbour, a neighbour at either end
// of the grid, v outside those three elements or outside the grid -- takes the whole range.
__device__ __forceinline__ int nearest_index_near(const double *a, double v, int n, int prev)
{
    int lo = 0, hi = n - 1;
    if (prev >= 1 && prev <= n - 2) {
        const double below = a[prev - 1], at = a[prev], above = a[prev + 1];
        if (below <= v && v < above) {
            lo = at > v ? prev - 1 : prev;
            hi = lo + 1;
        }
    }
    return pb::nearest_index(a, v, lo, hi);
}

// cutsteps = cutoff / dwnstep and inv_ofactor = 1.0 / ofactor are per-layer values prepared by
// k_layer_state (the same quotients the reference forms per line, _extcoeff.c:281-299).
// window_at(): the window from the group's sample idwn of the layer's grid, its sub-sample offset
// subw = iown - idwn * ofactor, its table cell and the cutoff's bounds mincut = (int)(idwn -
// cutsteps), maxcut = (int)(idwn + cutsteps) (used when the plan has a cutoff).
// kRec: the forms k_records takes (the quotients by an ofactor of 1 left out -- a wave-uniform
// branch -- and the others without a select), the same integers.
template <bool kRec>
__device__ __forceinline__ Window window_at(const LblArgs &a, int idwn, int subw, int cell,
                                            int ofactor, long dnwn, int mincut, int maxcut,
                                            double inv_ofactor, bool clip_lo, bool clip_hi)
{
    Window w;
    w.cell = cell;
    w.half = a.psize[cell];
    if (kRec && ofactor == 1) {
        w.minj = idwn - (w.half - subw);
        w.maxj = idwn + (w.half + subw);
    } else if (kRec) {
        w.minj = idwn - trunc_div_inv_abs(w.half - subw, inv_ofactor);
        w.maxj = idwn + trunc_div_inv_abs(w.half + subw, inv_ofactor);
    } else {
        w.minj = idwn - trunc_div_inv(w.half - subw, inv_ofactor);
        w.maxj = idwn + trunc_div_inv(w.half + subw, inv_ofactor);
    }
    // (the packed records of the staged gathers keep a window that leaves the grid unclipped:
    // see k_records)
    if (clip_lo && w.minj < 0)
        w.minj = 0;
    if (clip_hi && w.maxj > dnwn)
        w.maxj = dnwn;
    if (a.cutoff > 0.0) {
        if (mincut > w.minj)
            w.minj = mincut;
        if (maxcut < w.maxj)
            w.maxj = maxcut;
    }
    return w;
}

__device__ inline Window group_window(const LblArgs &a, double wavn, int iown, int ilor,
                                      double alphad, int ofactor, double dwnstep,
                                      int64_t dnwn, int idop_lo, int idop_hi,
                                      const double *doppler, double cutsteps,
                                      double inv_ofactor, bool clip_lo = true,
                                      bool clip_hi = true)
{
    // [idop_lo, idop_hi] brackets the answer (nearest index is monotonic in wavn), which
    // turns the bisection over the whole Doppler grid into 0-2 steps; `doppler` may point
    // to an LDS copy of the grid
    const int idwn = (int)((wavn - a.own0) / dwnstep);
    const int idop = idop_lo == idop_hi
                         ? idop_lo
                         : pb::nearest_index(doppler ? doppler : a.doppler, alphad * wavn,
                                             idop_lo, idop_hi);
    return window_at<false>(a, idwn, iown - idwn * ofactor, ilor * a.ndop + idop, ofactor,
                            (long)dnwn, (int)(idwn - cutsteps), (int)(idwn + cutsteps),
                            inv_ofactor, clip_lo, clip_hi);
}

// Co-added strength of a group (left-to-right sum of its members, _extcoeff.c:248-262)
__device__ inline double group_strength(const LblArgs &a, int first, int count, double ratio,
                                        double temp, double inv_temp, double z, double inv_z)
{
    double k = line_strength(ratio, a.gf[first], a.elow[first], a.lwn[first], temp, inv_temp, z,
                             inv_z);
    for (int m = 1; m < count; m++)
        k += line_strength(ratio, a.gf[first + m], a.elow[first + m], a.lwn[first + m],
                           temp, inv_temp, z, inv_z);
    return k;
}

__device__ inline void decode_block(const LblArgs &a, int &tile, int &layer)
{
    // blocks b and b+8 share an XCD: give each XCD its own layers, deepest first
    const int id = blockIdx.x;
    const int xcd = id & 7;
    const int k = id >> 3;
    tile = k % a.ntiles;
    const int grp = k / a.ntiles;
    // dealt to the XCDs in snake order (0..7, 7..0, ...): the cost of a layer falls with height,
    // and workgroup i always runs on XCD i % 8 -- dealt 0..7 every time, XCD 0 gets the heaviest
    // layer of every group of eight and finishes last (C3: 44.0 ms of work against 38.4 on XCD 6)
    const int rank = grp * 8 + ((grp & 1) ? 7 - xcd : xcd);
    layer = a.nlayers - 1 - rank;      // < 0 for the padding blocks
}

}  // namespace pbx
