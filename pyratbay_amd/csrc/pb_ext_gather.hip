// Line-by-line extinction, step 3 of the launch sequence (pb_extinction.hip) for constant-step
// grids: the global gather (k_ext_resample), the LDS-staged gather (k_ext_staged) with its split
// tables and k_combine_* passes, the resident-profile gather (k_ext_resident) and, in the
// experiments build, the scatter gather, the launch of the round gather and the probes of the
// staged kernel.  Which of them a call uses is plan_gather()'s decision (pb_extinction.hip).
//
// Global gather design (k_ext_resample, MI355X): a workgroup owns (layer, row, tile of 1024 output
// samples); a wavefront owns 4 consecutive 64-sample chunks and keeps their sums in
// registers, so every output is written exactly once, coalesced, without atomics and
// in a fixed order (bitwise reproducible).  Candidate groups of the tile are found by
// binary search in the (isotope, fine-index)-sorted group list; 256 of them at a time
// are turned -- one per lane -- into {strength, window, table offset} records in LDS
// (2 exp per group instead of per sample), then each wavefront walks the records that
// intersect its range (wave-level ballot culling).  The Voigt table is read through
// the phase-major layout of pb_voigt.hip: 64 lanes x 8 B contiguous per line chunk.
// Workgroups are numbered so that the 8 XCDs take different layers (the part of the
// table a layer touches -- one Lorentz row, a few Doppler columns -- then stays in
// that XCD's 4 MiB L2), heaviest (deepest) layers first.
#include <algorithm>
#include <climits>
#include <cmath>
#include <type_traits>
#include <vector>

#include "pb_ext_plan.h"

using namespace pbx;

namespace {

// ---------------------------------------------------------------------------
// 3a. gather, constant-step output grid (resample mode)
//
// Record of one candidate group (16 B in LDS): strength k, 32-bit table offset relative
// to a per-(workgroup, isotope) base pointer, window [lo, hi) packed as two 16-bit tile
// coordinates.  A lane owns the two consecutive samples c0 + 2*lane + {0,1} of each
// 128-sample chunk, so its byte offset from a record's table pointer is a per-lane
// CONSTANT: the load is `global_load_dwordx4 v, v_lane_off, s[tab]` with no per-record
// address arithmetic.  Lanes outside a record's window read whatever lies there (the
// table is padded by kTile samples on both sides, all finite); whether a chunk is
// fully inside (fma with the scalar k), partial (k or 0 selected per sample) or outside
// (skipped) is decided by scalar compares.
// ---------------------------------------------------------------------------
// RS wavefronts share one 256-sample range and split its records between them (each walks
// the records of every RS-th 64-record round); their partial sums are added in wavefront
// order through LDS.  RS > 1 shortens the critical path of a workgroup RS-fold -- used
// when the launch has too few workgroups to fill the chip (multi-GPU shards).
template <int RS, int NW>
__global__ __launch_bounds__(NW * 64) void k_ext_resample(LblArgs a)
{
    constexpr int NT = NW * 64;                  // threads = records per batch
    constexpr int kTileRS = (NW / RS) * kWaveSpan;   // output samples per workgroup
    static_assert(NW % RS == 0, "wavefronts must divide evenly into record shares");
    __shared__ double s_k[NT];
    __shared__ unsigned s_off[NT];
    __shared__ unsigned s_win[NT];               // lo | hi << 16

    int tile, layer;
    decode_block(a, tile, layer);
    if (layer < 0 || (a.res_cap > 0 && a.ls_resident[layer]))
        return;
    // launched beside the staged kernel (uneven line density): only the tiles it leaves out
    if (a.tsplit && a.tsplit[((int64_t)tile * kTileRS) / a.ts_tile] != 0)
        return;
    const int row = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    const int64_t t0 = a.wbegin + (int64_t)tile * kTileRS;         // global sample index
    const int64_t tend = min(t0 + kTileRS, a.wbegin + a.wcount);
    const int part = wave % RS;                                    // my share of the records
    const int rlo = (wave / RS) * kWaveSpan;                       // tile coordinates
    const int64_t recbase = (int64_t)layer * a.ngroups;
    const int rhi = (int)min((int64_t)rlo + kWaveSpan, tend - t0);

    const int ofactor = a.ls_ofactor[layer];
    const double kthresh =
        a.ethresh * __longlong_as_double((long long)a.kmax_bits[(int64_t)layer * a.nrows + row]);
    const int osamp = a.osamp;

    double acc[kChunks][kLaneSamples];
#pragma unroll
    for (int s = 0; s < kChunks; s++)
        acc[s][0] = acc[s][1] = 0.0;

    for (int iso = 0; iso < a.niso; iso++) {
        const int iext = a.isoiext[iso];
        if (iext < 0 || (a.add ? 0 : iext) != row)
            continue;
        const int64_t li = (int64_t)layer * a.niso + iso;
        const int ilor = a.li_ilor[li];
        const double alphad = a.li_alphad[li];
        const double dens = a.li_dens[li];
        int64_t reach = a.li_hmax[li];
        if (a.cutoff > 0.0)
            reach = min(reach, (int64_t)(a.cutoff / a.ownstep) + 2 * (int64_t)ofactor + 2);
        reach += osamp + ofactor;
        // groups whose window can touch [t0, tend)
        const int64_t seg0 = a.iso_gstart[iso], seg1 = a.iso_gstart[iso + 1];
        const int64_t g0 = lower_bound_i32(a.giown, seg0, seg1, t0 * osamp - reach);
        const int64_t g1 = lower_bound_i32(a.giown, seg0, seg1, (tend - 1) * osamp + reach + 1);
        if (g0 >= g1)
            continue;
        // Doppler-grid indices that the candidates can take: the nearest-index map is
        // monotonic in the line position, so it is bracketed by the images of the first
        // and last candidate positions (a leader lies within one fine step of own[iown]).
        const double vmin = a.own0 + ((double)a.giown[g0] - 1.0) * a.ownstep;
        // lowest Doppler column the candidates can use (their cells lie at or after it in
        // the table, so 32-bit offsets from its start are non-negative)
        const int idop_lo = pb::nearest_index(a.doppler, alphad * vmin, 0, a.ndop - 1);
        const int64_t cell_lo = (int64_t)ilor * a.ndop + idop_lo;
        const int64_t base_idx = a.pm_base[cell_lo] - kTile;       // inside the front pad
        const double *base = a.pm + base_idx;

        for (int64_t gb = g0; gb < g1; gb += NT) {
            __syncthreads();
            // ---- one record per lane: (layer, group) records from k_records ----
            {
                const int64_t g = gb + threadIdx.x;
                double k = 0.0;
                unsigned off = 0, win = 0;
                if (g < g1) {
                    int ulo, uhi, cell, phi, q;
                    if (a.tsplit) {
                        // the staged kernel's packed records (phase order): window end, row
                        // offset and phase follow from the cell's half-width and the position
                        const Rec16 r = a.rec16[(int64_t)layer * a.rec_pitch + a.pos2ph[g]];
                        k = r.k;
                        ulo = r.ulo;
                        uhi = ulo + (int)(r.lc & 0xfffu);
                        cell = (int)(r.lc >> 12);
                        const int d = a.psize[cell] - a.giown[g];          // half - iown
                        q = floor_div_inv(d, a.inv_osamp);
                        phi = d - q * osamp;
                    } else {
                        const int64_t idx = recbase + g;
                        k = a.rec_k[idx];
                        ulo = a.rec_ulo[idx];
                        uhi = a.rec_uhi[idx];
                        cell = a.rec_cell[idx];
                        phi = a.rec_phi[idx];
                        q = a.rec_q[idx];
                    }
                    const int64_t lo = max((int64_t)ulo, t0);
                    const int64_t hi = min((int64_t)uhi, tend);
                    if (!(k < kthresh) && lo < hi) {
                        if (a.add)
                            k *= dens;
                        win = (unsigned)(lo - t0) | ((unsigned)(hi - t0) << 16);
                        // tile sample j reads base[off + j]
                        off = (unsigned)(a.pm_base[cell] + (int64_t)phi * a.pm_stride[cell] + q +
                                         t0 - base_idx);
                        if (a.experiment == 1)
                            off = (unsigned)(kTile + (lo - t0));
                    } else {
                        k = 0.0;
                    }
                }
                s_k[threadIdx.x] = k;
                s_off[threadIdx.x] = off;
                s_win[threadIdx.x] = win;
            }
            __syncthreads();
            // ---- every wavefront walks the records that reach its samples ----
            const int nrec = a.experiment == 2 ? 0 : (int)min((int64_t)NT, g1 - gb);
            for (int b = 0; b < nrec; b += 64) {
                const int e = (b + lane) & (NT - 1);
                const unsigned my_win = s_win[e];
                // record g belongs to wavefront share (g / 64) % RS: a property of the
                // group, not of the tiling, so any tiling adds the same partial sums
                const bool mine = RS == 1 || (int)(((gb + b + lane) >> 6) & (RS - 1)) == part;
                const bool hit = mine && b + lane < nrec && (int)(my_win & 0xffff) < rhi &&
                                 (int)(my_win >> 16) > rlo;
                unsigned long long mask = __ballot(hit);
                const double my_k = s_k[e];
                const unsigned my_off = s_off[e];
                // kRecs records per trip: all loads are issued before the first fma
                while (mask) {
                    int src[kRecs];
#pragma unroll
                    for (int r = 0; r < kRecs; r++) {
                        src[r] = mask ? __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask))
                                      : -1;
                        mask &= mask - 1;        // no-op once mask is 0
                    }
                    double2 v[kRecs][kChunks];
                    double kk[kRecs];
                    int lo[kRecs], hi[kRecs];
#pragma unroll
                    for (int r = 0; r < kRecs; r++) {
                        const int sl = src[r] < 0 ? src[0] : src[r];
                        kk[r] = bcast(my_k, sl);
                        const unsigned win = (unsigned)__builtin_amdgcn_readlane((int)my_win, sl);
                        const unsigned off = (unsigned)__builtin_amdgcn_readlane((int)my_off, sl);
                        lo[r] = (int)(win & 0xffff);
                        hi[r] = (int)(win >> 16);
                        if (src[r] < 0)
                            kk[r] = 0.0;                                // padding slot
                        const double *tab = base + off;
#pragma unroll
                        for (int s = 0; s < kChunks; s++) {
                            // pair address clamped to [lo-1, hi-1]: in-window samples stay
                            // in their own slot, lanes outside re-read an edge line
                            const int j = rlo + s * kChunk + 2 * lane;
                            const int jc = min(max(j, lo[r] - 1), hi[r] - 1);
                            v[r][s] = *reinterpret_cast<const double2 *>(tab + jc);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < kRecs; r++) {
                        const unsigned span = (unsigned)(hi[r] - lo[r]);
#pragma unroll
                        for (int s = 0; s < kChunks; s++) {
                            const int j = rlo + s * kChunk + 2 * lane;
                            acc[s][0] = fma((unsigned)(j - lo[r]) < span ? kk[r] : 0.0,
                                            v[r][s].x, acc[s][0]);
                            acc[s][1] = fma((unsigned)(j + 1 - lo[r]) < span ? kk[r] : 0.0,
                                            v[r][s].y, acc[s][1]);
                        }
                    }
                }
            }
        }
    }

    if (RS > 1) {
        // partial sums of the wavefronts that share a range, added in wavefront order
        __shared__ double s_acc[NT * kChunks * kLaneSamples];
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kChunks; s++) {
            s_acc[(threadIdx.x * kChunks + s) * kLaneSamples + 0] = acc[s][0];
            s_acc[(threadIdx.x * kChunks + s) * kLaneSamples + 1] = acc[s][1];
        }
        __syncthreads();
        if (part != 0)
            return;
#pragma unroll
        for (int s = 0; s < kChunks; s++) {
            for (int q = 1; q < RS; q++) {
                const int t = threadIdx.x + q * 64;
                acc[s][0] += s_acc[(t * kChunks + s) * kLaneSamples + 0];
                acc[s][1] += s_acc[(t * kChunks + s) * kLaneSamples + 1];
            }
        }
    }
    double *dst = a.ext + ((int64_t)layer * a.nrows + row) * a.wcount + (t0 - a.wbegin);
#pragma unroll
    for (int s = 0; s < kChunks; s++) {
        const int j = rlo + s * kChunk + 2 * lane;
        if (j < rhi)
            dst[j] = acc[s][0];
        if (j + 1 < rhi)
            dst[j + 1] = acc[s][1];
    }
}

// ---------------------------------------------------------------------------
// 3a'. LDS-staged gather (constant-step grid), for line lists dense enough that several
// lines of a tile share one phase row of the Voigt table.
//
// Groups are visited in (isotope, phase key = iown mod osamp, iown) order.  All records
// with one (cell, phase, row window) key form a SEGMENT; the phase row is copied once
// into LDS -- zero outside the window, zero pads of kStagePad samples on both sides --
// and every record of the segment then adds k * row[j + q] to the samples it reaches
// with `ds_read_b64` + `v_fma_f64` and NO per-lane predicate: lanes beyond the window
// read zeros.  Compared with the global gather this moves each table sample through the
// texture path once per (tile, layer) instead of once per line, reads the operands at
// the LDS rate and executes ~1 VALU instruction per 64 samples.
// A lane owns the samples rlo + 64*c + lane (c < 4*G); a wavefront tests a record's
// window against groups of 4 chunks with scalar compares.
// ---------------------------------------------------------------------------

// NW wavefronts per workgroup, S sub-tiles of NW*256 samples each (tile = S*NW*256); one
// record per thread per batch.
// kProbe (timing experiments, results INVALID, never selected unless PB_STAGE_PROBE is set):
// 1 = "contiguous ownership": a lane owns 4 consecutive samples of a span and a visit is two
//     16-byte LDS reads at the 16-byte-aligned address at or below the one it needs (what a
//     second, 8-byte-shifted image of the row would make legal) instead of four 8-byte reads;
// 2 = the same with 2 consecutive samples per lane in each half of the span;
// 3 = (valid results) the remainder records of a visit loop software-pipelined;
// 4 = (valid results) the CYCLE ACCOUNT of a segment step: every
//     wavefront stamps s_memtime around the parts of its work and adds the differences, per layer,
//     to a.probe[layer * 24 + c]:  c = 0 candidate search and scans of an isotope, 1 record
//     fetch + decode of a batch (with its barriers), 2 segment detection + segment table (three
//     barriers), 3 find_hits (two bisections for 64 segments at once), 4 issue of a row's LDS-DMA
//     (the one wavefront whose turn it is), 5 the walk (hit decode, record broadcasts, row reads,
//     FMAs -- up to the last LDS value consumed), 6 s_waitcnt vmcnt(0) for the DMA, 7 the barrier
//     that ends the step, 8 pipeline fill of a batch (first row + barrier), 9 the wavefront's
//     lifetime, 10 segment steps, 11 batches, 12 (record, sub-tile) visits of this wavefront,
//     13 steps in which it visited anything, 14 accumulator read / write-back; calibration:
//     15 the lifetime on the 100-MHz wall clock (s_memrealtime), 16 two back-to-back stamp
//     intervals with an empty LDS queue, 17 wavefronts, 18 the interval of category 4 in the
//     wavefronts that did NOT request a row (a stamp right after a barrier release), 19 rows
//     requested, 20 the part of category 4 up to the first load (descriptor read + decode),
//     21 segments walked (a step, 10, is what ends at a barrier: up to kStageRowsMax segments).
//     A stamp is s_memtime + s_waitcnt lgkmcnt(0): it also drains the LDS queue, which is why
//     the probe is not the product kernel (profiles/r05_step_account.md gives both times).
// kIssue (kDma only): who requests a row's LDS-DMA.  0 = ONE wavefront per segment, the wavefronts
// taking turns, descriptor read and decoded at the time of the request (rounds 2-4); 1 = the same
// with the wavefront's NEXT descriptor fetched from LDS one turn (8 steps) ahead; 2 = EVERY
// wavefront requests its own 128-sample slice of the row (one load each), from a descriptor it
// fetched one step ahead.  Why: the cycle account (profiles/r05_step_account.md) shows the
// requesting wavefront ~700 cycles behind its peers in every step, who wait for it at the barrier.
// kRows (kDma, kIssue == 0): the most rows (segments) a barrier step stages.  1 = one row per step
// in two buffers; > 1 = stage_slots() (pb_ext_args.h) says per (layer, isotope) how many slots the
// same LDS holds, and a step stages and walks up to that many consecutive segments.  The sums are
// the same bits either way; plan_gather() / staged_kernel() choose.
template <int NW, int S, bool kDma, int kProbe = 0, int kIssue = 0, int kRows = 1>
__global__ __launch_bounds__(NW * 64, 8) void k_ext_staged(LblArgs a)
{
    constexpr int kThreads = NW * 64;
    constexpr int kSub = NW * kStageSpan;         // samples per sub-tile
    constexpr int kT = S * kSub;                  // samples per workgroup
    constexpr int kRowRegs = (kStageRowMax + kThreads - 1) / kThreads;
    static_assert(kT < 65536, "window coordinates are packed in 16 bits");
    extern __shared__ __align__(16) unsigned char smem[];
    const int osamp = a.osamp;
    // row buffers: [pad][row 0][pad][row 1][pad], pads of kStagePad zero samples shared
    double *s_row = reinterpret_cast<double *>(smem);
    struct __align__(16) Rec {
        double k;
        int qoff;                 // byte offset of tile sample 0 from the row buffer start
        unsigned win;             // lo | hi << 16 (tile coordinates)
    };
    const int rowspan = a.rowlds + kStagePad;                            // buffer pitch
    constexpr int kNB = 2;                        // row buffers
    Rec *s_rec = reinterpret_cast<Rec *>(s_row + kNB * rowspan + kStagePad);   // [kThreads]
    // LDS byte address of the records (taken once, as row_lds0): with a record's own offset it fits
    // the 16 bits a hit word has for it (find_hits), whatever the launch's rowlds <= kStageRowMax
    static_assert((kNB * (kStageRowMax + kStagePad) + kStagePad) * 8 + kThreads * 16 <= 65536,
                  "a hit word holds the LDS offset of a record in 16 bits");
    typedef double rec_v2 __attribute__((ext_vector_type(2)));
    typedef const rec_v2 rec_cv2;
    typedef __attribute__((address_space(3))) rec_cv2 *rec_lds_p;
    const unsigned rec_off0 =
        (unsigned)(size_t)(__attribute__((address_space(3))) char *)(reinterpret_cast<char *>(s_rec));
    long long *s_src = reinterpret_cast<long long *>(s_rec + kThreads);  // row start, -1 empty
    unsigned long long *s_desc = reinterpret_cast<unsigned long long *>(s_src);   // per segment
    unsigned long long *s_segmask =
        reinterpret_cast<unsigned long long *>(s_src + kThreads);        // [NW]
    unsigned *s_m = reinterpret_cast<unsigned *>(s_segmask + NW);        // mlo | mhi << 16
    // the segment table takes the place of the window keys, which nothing reads once the
    // segment starts are known (a barrier lies between the last read and the first write)
    unsigned *s_seg = s_m;                                               // i0 | i1 << 16
    // the table cells of this (layer, isotope): one Lorentz row, ndop Doppler columns
    long long *s_cbase = reinterpret_cast<long long *>(s_m + kThreads);  // [ndop] pm_base
    int *s_csize = reinterpret_cast<int *>(s_cbase + a.ndop);            // [ndop] psize
    int *s_cstride = s_csize + a.ndop;                                   // [ndop] pm_stride
    int *s_part = s_cstride + a.ndop;                                    // [NW] scan scratch
    const int vmax = osamp * a.nch_max;                                  // (phase, chunk) pairs
    int *s_cum = s_part + NW;                                            // [vmax+1]
    int *s_phs = s_cum + (vmax + 1);                                     // [vmax]

    // Blocks b and b+8 share an XCD.  The unit handed to an XCD is a (layer, phase split)
    // pair, deepest layer first: the splits of one layer read different phase rows, so
    // spreading them over the XCDs costs no L2 sharing, and a launch of few layers (a
    // multi-GPU rank: 10 layers on 8 XCDs) still loads every XCD alike.
    int tile, layer, zsplit;
    {
        const int id = blockIdx.x;
        const int k = id >> 3;
        tile = k % a.ntiles;
        const int grp = k / a.ntiles;                  // snake order over the XCDs: decode_block
        const int unit = grp * 8 + ((grp & 1) ? 7 - (id & 7) : (id & 7));
        if (a.unit_tab) {
            // per-layer split: the unit table lists the (layer, piece) pairs, deepest layer first
            const int e = unit < a.nunits ? a.unit_tab[unit] : -1;
            layer = e < 0 ? -1 : e >> 8;
            zsplit = e & 0xff;
        } else {
            layer = a.nlayers - 1 - unit / a.nsplit;   // < 0 for the padding blocks
            zsplit = unit % a.nsplit;
        }
    }
    if (layer < 0 || (a.res_cap > 0 && a.ls_resident[layer]) || (a.wave_cap > 0 && a.ls_wave[layer]))
        return;
    // pieces of this tile: per layer, per tile (uneven line density) or one number for the launch
    const int nsp = a.tsplit ? a.tsplit[tile] : a.lsplit ? a.lsplit[layer] : a.nsplit;
    if (zsplit >= nsp)
        return;
    const int row = blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned long long pc[22] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto tick = [&]() -> unsigned long long {
        if constexpr (kProbe == 4)
            return (unsigned long long)__builtin_amdgcn_s_memtime();
        return 0ull;
    };
    unsigned long long real_birth = 0;
    if constexpr (kProbe == 4) {
        // calibration: the cost of a stamp with an empty LDS queue (16 = three stamps in a row,
        // i.e. two intervals; 17 = 1) and the 100-MHz wall clock beside s_memtime (15)
        real_birth = (unsigned long long)__builtin_amdgcn_s_memrealtime();
        const unsigned long long c0 = tick();
        const unsigned long long c1 = tick();
        const unsigned long long c2 = tick();
        pc[16] = (c2 - c0) + 0 * c1;
        pc[17] = 1;
    }
    const unsigned long long t_birth = tick();

    const int64_t t0 = a.wbegin + (int64_t)tile * kT;
    const int64_t tend = min(t0 + kT, a.wbegin + a.wcount);
    const int tlen = (int)(tend - t0);
    const int rlo = wave * kStageSpan;            // first sample of sub-tile 0 (tile coords)

    // (wave-uniform numbers that a vector load brought: kept in scalar registers, or they are
    // spilled to scratch around the step loop)
    auto uniform = [](double x) {
        return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)),
                                __builtin_amdgcn_readfirstlane(__double2loint(x)));
    };
    const double kthresh = uniform(
        a.ethresh * __longlong_as_double((long long)a.kmax_bits[(int64_t)layer * a.nrows + row]));
    // packed records of this layer, indexed by the position in the phase-sorted group list
    const int64_t recbase = a.rec16 ? (int64_t)layer * a.rec_pitch - a.grp_lo
                                    : (int64_t)layer * a.ngroups;
    double *const out = zsplit == 0
                            ? a.ext
                            : a.part + (int64_t)(zsplit - 1) * a.nlayers * a.nrows * a.wcount;
    double *const dst = out + ((int64_t)layer * a.nrows + row) * a.wcount + (t0 - a.wbegin);

    double acc[S][4];
#pragma unroll
    for (int u = 0; u < S; u++)
        acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.0;
    if (a.accumulate) {
        // a later chunk of the line list: go on from the running sums of the earlier ones
#pragma unroll
        for (int u = 0; u < S; u++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int j = rlo + u * kSub + c * 64 + lane;
                if (j < tlen)
                    acc[u][c] = dst[j];
            }
    }
    for (int i = tid; i < kNB * rowspan + kStagePad; i += kThreads)
        s_row[i] = 0.0;                            // the pads stay zero for good

    // Row of one segment -> registers (issued early), registers -> LDS (after the walk).
    // The registers form a ring of D sets of R doubles per lane (D*R = 2*kRowRegs): rows
    // that fit one register per lane (<= kThreads samples) are fetched 4 segments ahead.
    double ring[kDma ? 1 : 2 * kRowRegs];
    // Rows of this (layer, isotope) are at most `rowlim` samples long: wavefronts whose
    // lanes lie beyond it do not store (the buffers are zeroed per isotope).
    int rowlim = a.rowlds;
    // kRows > 1: `nrow` rows per barrier step in slots of `pitch` samples (stage_slots(),
    // pb_ext_args.h), set with rowlim; every other instance keeps one row per step, two buffers
    constexpr bool kMulti = kDma && kIssue == 0 && kRows > 1;
    int pitch = rowspan, nrow = 1;
    // The product instances fold a segment's slot into the row offsets of its records
    // (stage_slot_off8(), pb_ext_args.h), so their walk reads every segment from the lane's address
    // in slot 0.  The register path and the kIssue / kProbe forms add the buffer's offset to the
    // lane's address per segment instead: the independent statement of the same addresses.
    constexpr bool kFold = kDma && kIssue == 0 && kProbe == 0;
    static_assert(kRows <= kStageRowsMax && kStageRowsMax <= NW,
                  "a wavefront requests at most one row of a step");
    // kDma: the row of a segment goes global -> LDS directly (`buffer_load_dwordx4 ... lds`,
    // 1 KiB = 128 samples per wave-instruction), issued by ONE wavefront per segment (the
    // wavefronts take turns), one step ahead of the walk.  No row registers, no LDS stores
    // and one descriptor chain per workgroup and segment instead of eight.  Lanes outside
    // the window read 0 through the buffer range check (checked per dword at the upper end;
    // a lane below the window is out of range as a whole, so the LDS image is shifted by the
    // parity e of the window start -- row sample m sits at position m - e, which the
    // records' offsets account for -- and no lane straddles the lower edge).  The
    // instruction is issued from inline asm: the compiler would otherwise drain it
    // (vmcnt(0)) before the next LDS read; the wait before the barrier is explicit.
    // LDS byte address of row buffer 0 (taken once: the flat -> LDS cast of a pointer the compiler
    // cannot prove non-null costs a compare per use, and trips a register-class bug of this
    // compiler when the lambda below is instantiated for several call sites)
    const unsigned row_lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)(
        reinterpret_cast<char *>(s_row + kStagePad));
    //
    // The request of a whole row.  For a MUBUF load with the `lds` bit the 12-bit `offset:` field
    // of the instruction is added on BOTH sides: memory address = base + voffset + offset (range
    // checked against the descriptor as before), LDS address = LDS base + M0[15:0] + offset +
    // lane * 16.  Consecutive 1-KiB pieces of a row differ by +1024 on both sides, so pieces 0..3
    // are four loads with offset:0/1024/2048/3072 behind ONE write of M0, and pieces 4..7 the same
    // behind a second one (M0 and voffset + 4096): no address arithmetic, compare or branch per
    // piece.  M0 is written in the statement that reads it (the compiler does not keep it).
    // `s_nop 4` opens the first statement of a request: the descriptor's SGPRs come from
    // v_readfirstlane, and a VALU write of an SGPR needs five wait states before a VMEM
    // instruction reads it; the hazard does apply here (the s_mov of M0 is an SALU read and
    // would need none, the load does), and hipcc pads nothing inside a statement.  The second
    // statement of a request follows the first in program order (both volatile) with the same
    // descriptor registers, at least eight instructions later, and needs none.
    // The number of pieces is EXACT, ceil(rowlim / 128): a piece writes all of its 128 samples
    // (zeros beyond the descriptor's range), which the pad after a slot absorbs for the last
    // piece of a row (tests/test_rows_per_step_cpu.py) but not for a surplus one -- with two rows
    // per step (pitch = rowlim + 256) that would reach the data of the next slot.  It is formed
    // where rowlim is (`npiece`), wave-uniform, and selects the statement by a scalar switch.
    int npiece = (rowlim + 127) >> 7;              // 0 ... 8
    typedef int dma_v4i __attribute__((ext_vector_type(4)));
#define PB_DMA_OPEN "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
#define PB_DMA_LD(off) "buffer_load_dwordx4 %2, %3, 0 offen offset:" #off " lds\n\t"
#define PB_DMA_LD1 PB_DMA_LD(0)
#define PB_DMA_LD2 PB_DMA_LD1 PB_DMA_LD(1024)
#define PB_DMA_LD3 PB_DMA_LD2 PB_DMA_LD(2048)
#define PB_DMA_LD4 PB_DMA_LD3 PB_DMA_LD(3072)
#define PB_DMA_GROUP(pad, loads, dst_, voff_)                                                    \
    do {                                                                                         \
        unsigned keep;                                                                           \
        asm volatile(pad PB_DMA_OPEN loads "s_mov_b32 m0, %0"                                    \
                     : "=&s"(keep)                                                               \
                     : "s"(dst_), "v"(voff_), "s"(rsrc)                                          \
                     : "memory");                                                                \
    } while (0)
    auto dma_pieces = [&](unsigned dst, int voff, dma_v4i rsrc) {
        const unsigned dst4 = dst + 4096;
        const int voff4 = voff + 4096;
        switch (npiece) {                          // wave-uniform
        case 1: PB_DMA_GROUP("s_nop 4\n\t", PB_DMA_LD1, dst, voff); break;
        case 2: PB_DMA_GROUP("s_nop 4\n\t", PB_DMA_LD2, dst, voff); break;
        case 3: PB_DMA_GROUP("s_nop 4\n\t", PB_DMA_LD3, dst, voff); break;
        case 4: PB_DMA_GROUP("s_nop 4\n\t", PB_DMA_LD4, dst, voff); break;
        case 5:
            PB_DMA_GROUP("s_nop 4\n\t", PB_DMA_LD4, dst, voff);
            PB_DMA_GROUP("", PB_DMA_LD1, dst4, voff4);
            break;
        case 6:
            PB_DMA_GROUP("s_nop 4\n\t", PB_DMA_LD4, dst, voff);
            PB_DMA_GROUP("", PB_DMA_LD2, dst4, voff4);
            break;
        case 7:
            PB_DMA_GROUP("s_nop 4\n\t", PB_DMA_LD4, dst, voff);
            PB_DMA_GROUP("", PB_DMA_LD3, dst4, voff4);
            break;
        case 8:
            PB_DMA_GROUP("s_nop 4\n\t", PB_DMA_LD4, dst, voff);
            PB_DMA_GROUP("", PB_DMA_LD4, dst4, voff4);
            break;
        default: break;                            // no row data in this (layer, isotope)
        }
    };
#undef PB_DMA_GROUP
#undef PB_DMA_LD4
#undef PB_DMA_LD3
#undef PB_DMA_LD2
#undef PB_DMA_LD1
#undef PB_DMA_LD
#undef PB_DMA_OPEN
    // (tref, probe 4: the stamp that opened the step -- the descriptor chain is timed against it)
    // `boff`: byte offset of the row's buffer (or slot) from buffer 0.
    // `part`: true_type = the pieces [c_lo, c_hi) of the row only, one statement per piece (the
    // kIssue == 2 experiment); false_type = the whole row through dma_pieces()
    auto dma_desc = [&](unsigned long long d, unsigned boff, auto part, int c_lo, int c_hi,
                        unsigned long long tref = 0) {
        const unsigned dlo = (unsigned)__builtin_amdgcn_readfirstlane((int)d);
        const unsigned dhi = (unsigned)__builtin_amdgcn_readfirstlane((int)(d >> 32));
        const long long first = ((long long)(dhi & 0xffu) << 32) | dlo;
        const int len = (int)((dhi >> 8) & 0xfffu), mlo = (int)(dhi >> 20);
        const unsigned long long base = (unsigned long long)(a.pm + first);
        dma_v4i rsrc;
        rsrc.x = __builtin_amdgcn_readfirstlane((int)base);
        rsrc.y = __builtin_amdgcn_readfirstlane((int)((base >> 32) & 0xffffu));
        rsrc.z = __builtin_amdgcn_readfirstlane(len * 8);
        rsrc.w = 0x00020000;
        int voff = (2 * lane - (mlo & ~1)) * 8;
        unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)(row_lds0 + boff));
        if constexpr (kProbe == 4) {
            if (tref)
                pc[20] += tick() - tref;
        }
        if constexpr (!decltype(part)::value) {
            dma_pieces(dst, voff, rsrc);
        } else {
            voff += 1024 * c_lo;
            dst += 1024 * (unsigned)c_lo;
            for (int c = c_lo; c < c_hi && c * 128 < rowlim; c++) {
                unsigned keep;
                asm volatile("s_nop 4\n\t"
                             "s_mov_b32 %0, m0\n\t"
                             "s_mov_b32 m0, %1\n\t"
                             "s_nop 0\n\t"
                             "buffer_load_dwordx4 %2, %3, 0 offen lds\n\t"
                             "s_mov_b32 m0, %0"
                             : "=&s"(keep)
                             : "s"(dst), "v"(voff), "s"(rsrc)
                             : "memory");
                voff += 1024;
                dst += 1024;
            }
        }
    };
    auto bufoff = [&](int buf) { return (unsigned)(buf * rowspan * 8); };   // one row per step
    auto dma_row = [&](int sg, unsigned boff, unsigned long long tref = 0) {
        dma_desc(s_desc[sg], boff, std::false_type(), 0, 0, tref);
    };
    // out-of-window lanes fall outside the buffer descriptor and read 0 (no predicate)
    auto load_row = [&](int sg, auto Rc, double *reg) {
        constexpr int R = decltype(Rc)::value;
        const unsigned long long d = s_desc[sg];
        const unsigned dlo = (unsigned)__builtin_amdgcn_readfirstlane((int)d);
        const unsigned dhi = (unsigned)__builtin_amdgcn_readfirstlane((int)(d >> 32));
        const long long first = ((long long)(dhi & 0xffu) << 32) | dlo;
        const int len = (int)((dhi >> 8) & 0xfffu), mlo = (int)(dhi >> 20);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(a.pm + first), 0, len * 8, 0x00020000);
        typedef int v2i __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int r = 0; r < R; r++) {
            const v2i v = __builtin_amdgcn_raw_buffer_load_b64(
                rsrc, (tid + r * kThreads - mlo) * 8, 0, 0);
            reg[r] = __hiloint2double(v.y, v.x);
        }
    };
    auto store_row = [&](int buf, auto Rc, const double *reg, auto Dc) {
        constexpr int R = decltype(Rc)::value;
        // The (D-1)*R loads issued after this set stay in flight.  The wait is explicit and
        // unconditional: left to the conditional stores below, the path that skips them
        // reaches the loop header with the set still pending and the compiler drains the
        // whole prefetch queue (vmcnt(0)) at the top of every other segment.
        constexpr int kInFlight = (decltype(Dc)::value - 1) * R;
        __builtin_amdgcn_s_waitcnt((kInFlight & 0xf) | (0x7 << 4) | (0xf << 8) |
                                   ((kInFlight >> 4) << 14));
        double *dst = s_row + kStagePad + buf * rowspan;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (wave * 64 + r * kThreads >= rowlim)
                continue;
            const int mm = tid + r * kThreads;
            if (mm < a.rowlds)
                dst[mm] = reg[r];
        }
    };

    pc[14] += tick() - t_birth;
    for (int iso = 0; iso < a.niso; iso++) {
        const int iext = a.isoiext[iso];
        if (iext < 0 || (a.add ? 0 : iext) != row)
            continue;
        if ((iso + 1) * osamp <= a.key_lo || iso * osamp >= a.key_hi)
            continue;                              // no key of this isotope in the chunk
        const unsigned long long t_iso = tick();
        const int64_t li = (int64_t)layer * a.niso + iso;
        const double dens = uniform(a.li_dens[li]);
        int64_t reach = a.li_hmax[li];
        if (a.cutoff > 0.0)
            reach = min(reach, (int64_t)(a.cutoff / a.ownstep) + 2 * (int64_t)a.ls_ofactor[layer] + 2);
        reach += osamp + a.ls_ofactor[layer];
        const int64_t flo = t0 * osamp - reach, fhi = (tend - 1) * osamp + reach;

        // candidates of every phase key: [s_phs[p], s_phs[p] + count) in the phase list,
        // then an exclusive scan of the counts (thread t owns a run of `per` phases)
        __syncthreads();
        // first cell of the isotope's Lorentz row (wave-uniform: kept in a scalar register)
        const int cell0 = __builtin_amdgcn_readfirstlane(a.li_ilor[li] * a.ndop);
        for (int d = tid; d < a.ndop; d += kThreads) {
            s_cbase[d] = a.pm_base[cell0 + d];
            s_csize[d] = a.psize[cell0 + d];
            s_cstride[d] = a.pm_stride[cell0 + d];
        }
        {
            const int lim = min(a.rowlds, a.li_rowmax[li]);
            if (lim != rowlim) {                   // wave-uniform
                for (int i = tid; i < kNB * rowspan + kStagePad; i += kThreads)
                    s_row[i] = 0.0;
                rowlim = lim;
                npiece = (lim + 127) >> 7;
                if constexpr (kMulti) {
                    const StageSlots sl = stage_slots(a.rowlds, lim, min(kRows, a.rows_cap));
                    // (wave-uniform, but formed from a vector load: said so, or the step loop's
                    // arithmetic on them is done by the vector unit and read back)
                    pitch = __builtin_amdgcn_readfirstlane(sl.pitch);
                    nrow = __builtin_amdgcn_readfirstlane(sl.rows);
                }
            }
        }
        // "virtual phases": (phase p, chunk c) pairs, pv = p*nch + c; nch = 1 unless the rows of
        // this (layer, isotope) are longer than kStageRowMax
        const int nch = a.nch_max > 1
                            ? (min(a.rowcap, a.li_rowmax[li]) + kChunkRow - 1) / kChunkRow
                            : 1;
        const int nvirt = osamp * nch;
        const int per = (nvirt + kThreads - 1) / kThreads;
        int mine = 0;
        for (int r = 0; r < per; r++) {
            const int pv = tid * per + r;
            const int p = pv / nch, c = pv - p * nch;
            if (pv < nvirt && ((nsp > 1 && p * nsp / osamp != zsplit) ||
                               iso * osamp + p < a.key_lo || iso * osamp + p >= a.key_hi)) {
                s_phs[pv] = 0;                     // another workgroup's, or another chunk's, phase
                s_cum[pv] = 0;
            } else if (pv < nvirt) {
                // two table lookups bracket each bound to within one bin (a fraction of a
                // record per phase), then a short bisection makes it exact
                const int32_t *bin = a.ph_bin + ((int64_t)iso * osamp + p) * (a.ph_nbins + 1);
                const int64_t binw = (int64_t)kBinSamples * osamp;
                // a chunk of a long row covers the samples [c0 - q, c0 + 1024 - q) with
                // q = floor((half - iown)/osamp): only groups at fine positions within
                // [t0*osamp + half - (c0+1024)*osamp, tend*osamp + half - c0*osamp] (+- one
                // sample, half between the smallest and largest one of the isotope) reach the tile
                int64_t clo = flo, chi = fhi;
                if (a.nch_max > 1) {
                    const int64_t c0 = (int64_t)c * kChunkRow;
                    clo = max(clo, (t0 - c0 - kChunkRow - 1) * osamp + a.li_hlo[li]);
                    chi = min(chi, (tend - c0 + 1) * osamp + a.li_hhi[li]);
                    if (chi < clo)
                        chi = clo - 1;
                }
                const int b0 = (int)min((int64_t)a.ph_nbins - 1, max((int64_t)0, clo) / binw);
                const int b1 = (int)min((int64_t)a.ph_nbins - 1, max((int64_t)0, chi + 1) / binw);
                const int32_t l0 = bin[b0], h0 = bin[b0 + 1], l1 = bin[b1], h1 = bin[b1 + 1];
                int64_t s0, s1;
                lower_bound2_i32(a.ph_iown, l0, h0, clo, l1, h1, chi + 1, s0, s1);
                s_phs[pv] = (int)s0;               // entry of the layer's record array
                s_cum[pv] = (int)(s1 - s0);
                mine += (int)(s1 - s0);
            }
        }
        int incl = mine;                           // inclusive scan inside the wavefront
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d)
                incl += up;
        }
        if (lane == 63)
            s_part[wave] = incl;
        __syncthreads();
        int base = 0, total = 0;
        for (int w = 0; w < NW; w++) {
            const int pw = s_part[w];
            if (w < wave)
                base += pw;
            total += pw;
        }
        int run = base + incl - mine;
        for (int r = 0; r < per; r++) {
            const int pv = tid * per + r;
            if (pv < nvirt) {
                const int c = s_cum[pv];
                s_cum[pv] = run;
                run += c;
            }
        }
        if (tid == 0)
            s_cum[nvirt] = total;
        __syncthreads();
        pc[0] += tick() - t_iso;

        for (int x0 = 0; x0 < total; x0 += kThreads) {
            const int nrec = min(kThreads, total - x0);
            const unsigned long long t_batch = tick();
            pc[11] += 1;
            __syncthreads();
            // ---- one record per lane, in (phase, iown) order, from k_records ----
            long long src = -1;                        // phase row of my record (table element)
            unsigned mwin = 0;                         // its window in row coordinates
            // {k, qoff, win} of my record: stored behind the segment detection, which says in
            // which slot the record's row will lie
            double k = 0.0;
            unsigned win = 0;
            int qoff = 0;
            {
                const int x = x0 + tid;
                if (x < total) {
                    int plo = 0, pup = nvirt;           // largest pv with s_cum[pv] <= x
                    while (pup - plo > 1) {
                        const int mid = (plo + pup) >> 1;
                        if (s_cum[mid] <= x)
                            plo = mid;
                        else
                            pup = mid;
                    }
                    const int64_t entry = s_phs[plo] + (x - s_cum[plo]);
                    const int64_t gidx = entry;         // index in the phase-sorted group list
                    int c0 = 0;                         // first row sample of my chunk
                    if (a.nch_max > 1)
                        c0 = (plo % nch) * kChunkRow;
                    const int64_t idx = recbase + entry;
                    int ulo, uhi, q, cell, phi;
                    if (a.rec16) {
                        const Rec16 r = a.rec16[idx];
                        k = r.k;
                        ulo = r.ulo;
                        const int lbits = a.nch_max > 1 ? kLongLenBits : 12;
                        uhi = ulo + (int)(r.lc & ((1u << lbits) - 1u));
                        cell = (int)(r.lc >> lbits);
                        const int d = s_csize[cell - cell0] - a.ph_iown[gidx];   // half - iown
                        q = floor_div_inv(d, a.inv_osamp);
                        phi = d - q * osamp;
                        if (a.nch_max > 1) {
                            // the part of the window whose row coordinates u = sample + q fall
                            // into my chunk [c0, c0 + kChunkRow)
                            const int wlo = max(ulo + q, c0), whi = min(uhi + q, c0 + kChunkRow);
                            if (whi > wlo) {
                                ulo = wlo - q;
                                uhi = whi - q;
                            } else {
                                uhi = ulo;
                            }
                        }
                        q -= c0;                        // row index relative to the chunk
                    } else {
                        k = a.rec_k[idx];
                        ulo = a.rec_ulo[idx];
                        uhi = a.rec_uhi[idx];
                        q = a.rec_q[idx];
                        cell = a.rec_cell[idx];
                        phi = a.rec_phi[idx];
                    }
                    const int lo = (int)(max((int64_t)ulo, t0) - t0);
                    const int hi = (int)(min((int64_t)uhi, tend) - t0);
                    if (!(k < kthresh) && lo < hi) {
                        if (a.add)
                            k *= dens;
                        win = (unsigned)lo | ((unsigned)hi << 16);
                        qoff = (int)(q + t0) * 8;       // tile sample j reads row[j + q + t0]
                        if (kDma)
                            qoff -= ((ulo + q) & 1) * 8;  // the image starts at an even sample
                        src = s_cbase[cell - cell0] + (long long)phi * s_cstride[cell - cell0] + c0;
                        mwin = (unsigned)(ulo + q) | ((unsigned)(uhi + q) << 16);
                    } else {
                        k = 0.0;
                    }
                }
                s_src[tid] = src;
                s_m[tid] = mwin;
            }
            __syncthreads();
            const unsigned long long t_seg = tick();
            pc[1] += t_seg - t_batch;
            // ---- segments: runs of equal (cell, phase, row window); live ones are listed ----
            bool start = false;
            {
                if (tid < nrec)
                    start = tid == 0 || s_src[tid] != s_src[tid - 1] || s_m[tid] != s_m[tid - 1];
                const unsigned long long m = __ballot(start);
                if (lane == 0)
                    s_segmask[wave] = m;
            }
            const bool live = start && s_src[tid] >= 0;
            const unsigned long long livemask = __ballot(live);
            if (lane == 0)
                s_part[wave] = __builtin_popcountll(livemask);
            __syncthreads();
            int nseg = 0;
            {
                int before = 0;
                for (int w = 0; w < NW; w++) {
                    const int c = s_part[w];
                    if (w < wave)
                        before += c;
                    nseg += c;
                }
                // live segment starts in the lanes below mine
                const int below = (int)__builtin_amdgcn_mbcnt_hi(
                    (unsigned)(livemask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)livemask, 0u));
                // My record goes to LDS, with the slot of its segment folded into its row offset
                // (kFold).  A live record's segment is the last live start at or before it --
                // before + below, less one where the start is not mine; a record behind a dead
                // start is dead itself (k = 0, an empty window: no pair holds it) and its offset
                // is never used.
                if constexpr (kFold)
                    qoff += (int)stage_slot_off8(before + below - (live ? 0 : 1), nrow,
                                                 (unsigned)pitch * 8u);
                s_rec[tid].k = k;
                s_rec[tid].qoff = qoff;
                s_rec[tid].win = win;
                if (live) {
                    // end of my segment = next start after me
                    int w = tid >> 6;
                    unsigned long long m = s_segmask[w] & ~((2ull << (tid & 63)) - 1ull);
                    int end = nrec;
                    for (;;) {
                        if (m) {
                            end = min(nrec, w * 64 + (int)__builtin_ctzll(m));
                            break;
                        }
                        if (++w >= NW)
                            break;
                        m = s_segmask[w];
                    }
                    const int pos = before + below;
                    s_seg[pos] = (unsigned)tid | ((unsigned)end << 16);
                    // the row descriptor of the segment, packed: first element of the window
                    // (40 bits) | window length << 40 (12 bits) | window start << 52 (12 bits).
                    // It overwrites s_src, which nothing reads after the barrier above.
                    const unsigned long long mlo = mwin & 0xffffu, mhi = mwin >> 16;
                    s_desc[pos] = (unsigned long long)(src + (long long)mlo) | ((mhi - mlo) << 40) |
                                  (mlo << 52);
                }
            }
            __syncthreads();
            pc[2] += tick() - t_seg;
            if (nseg == 0)
                continue;
            // ---- rows are double-buffered in LDS and fetched two segments ahead: segment
            // sg+2's row is already in flight (in registers) while sg is walked, and is
            // written to the free LDS buffer one segment later ----
            // Lane l of every wavefront keeps, for segment (sg & ~63) + l, the records that
            // reach each of the wavefront's sub-tiles: first | count << 16.  The records of a
            // segment have equal window lengths and ascending positions, so those are
            // consecutive and two bisections find them; 64 segments are done at once.
            unsigned hits[S];
            auto find_hits = [&](int sg0) {
                const int sgl = sg0 + lane;
                const unsigned sd = sgl < nseg ? s_seg[sgl] : 0u;
                const int i0 = (int)(sd & 0xffff), i1 = (int)(sd >> 16);
#pragma unroll
                for (int u = 0; u < S; u++) {
                    const int slo = rlo + u * kSub;
                    int lo = i0, hi = i1;              // first record with window end > slo
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if ((int)(s_rec[mid].win >> 16) > slo)
                            hi = mid;
                        else
                            lo = mid + 1;
                    }
                    const int first = lo;
                    hi = i1;                           // first record starting at or after the end
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if ((int)(s_rec[mid].win & 0xffff) >= slo + kStageSpan)
                            hi = mid;
                        else
                            lo = mid + 1;
                    }
                    // what the walk uses, ready made: the LDS byte address of the first record
                    // << 16 | the bytes of the pair's four-record trips (a multiple of 64) | the
                    // 0-3 records left after them; 0 = no record
                    const unsigned n = (unsigned)(lo - first);
                    hits[u] = slo < tlen && n
                                  ? (rec_off0 + (unsigned)first * 16u) << 16 | (n & ~3u) << 4 | (n & 3u)
                                  : 0u;
                }
            };
            // the hit words of the 64 segments from sg on (sg: a multiple of 64)
            auto block_hits = [&](int sg) {
                const unsigned long long tf = tick();
                find_hits(sg);
                pc[3] += tick() - tf;
            };
            // `rowp`: byte address of this lane's first sample in the staged row of the segment
            auto walk_row = [&](int sg, const char *rowp) {
                bool any = false;
#pragma unroll
                for (int u = 0; u < S; u++) {
                    const unsigned h = (unsigned)__builtin_amdgcn_readlane((int)hits[u], sg & 63);
                    if (h == 0u)
                        continue;
                    if constexpr (kProbe == 4) {
                        pc[12] += ((h & 0xffc0u) >> 4) + (h & 3u);
                        any = true;
                    }
                    // per record: ONE 16-byte broadcast read of {k, offset, window}, four
                    // 64-sample row reads, four fma; four records per trip
                    const char *rs = rowp + (size_t)u * kSub * 8;
                    rec_lds_p recs = (rec_lds_p)(size_t)(h >> 16);
                    const rec_lds_p trips_end = (rec_lds_p)(size_t)((h >> 16) + (h & 0xffc0u));
                    auto visit = [&](const rec_v2 raw) {
                        const double k = raw.x;
                        const int qoff = __double2loint(raw.y);
                        if constexpr (kProbe == 1 || kProbe == 2) {
                            // 1: 4 consecutive samples per lane (lane pitch 32 B: two-way bank
                            // conflicts); 2: 2 consecutive samples in each half of the span (lane
                            // pitch 16 B, conflict-free)
                            // (offsets from the LDS base: a pointer rebuilt from an integer
                            // would be a flat pointer and the reads flat loads)
                            const char *base = reinterpret_cast<const char *>(s_row);
                            const int off = ((int)(rs - base) + (kProbe == 1 ? 3 : 1) * 8 * lane + qoff) & ~15;
                            const double2 v0 = *reinterpret_cast<const double2 *>(base + off);
                            const double2 v1 = *reinterpret_cast<const double2 *>(
                                base + off + (kProbe == 1 ? 16 : 1024));
                            acc[u][0] = fma(k, v0.x, acc[u][0]);
                            acc[u][1] = fma(k, v0.y, acc[u][1]);
                            acc[u][2] = fma(k, v1.x, acc[u][2]);
                            acc[u][3] = fma(k, v1.y, acc[u][3]);
                            return;
                        }
                        const double *p0 = reinterpret_cast<const double *>(rs + qoff);
                        const double a0 = p0[0], a1 = p0[64], a2 = p0[128], a3 = p0[192];
                        acc[u][0] = fma(k, a0, acc[u][0]);
                        acc[u][1] = fma(k, a1, acc[u][1]);
                        acc[u][2] = fma(k, a2, acc[u][2]);
                        acc[u][3] = fma(k, a3, acc[u][3]);
                    };
                    // the trips loop on the record address alone
                    for (; recs != trips_end; recs += 4) {
                        const rec_v2 w0 = recs[0], w1 = recs[1], w2 = recs[2], w3 = recs[3];
                        visit(w0);
                        visit(w1);
                        visit(w2);
                        visit(w3);
                    }
                    const int left = (int)(h & 3u);
                    if constexpr (kProbe == 3) {
                        // remainder records software-pipelined: the next record's {k, offset} is
                        // requested before the current record's row reads are consumed
                        if (left) {
                            rec_v2 cur = recs[0];
                            for (int r = 1; r < left; r++) {
                                const rec_v2 nxt = recs[r];
                                visit(cur);
                                cur = nxt;
                            }
                            visit(cur);
                        }
                    } else {
                        // the 0-3 records left, in record order: one if the count is odd, then
                        // two (read together, immediate offsets 0 / 16) if its bit 1 is set.  No
                        // loop and no padding record; two branches that skip forward and no
                        // if / else, which the structuriser would rebuild with copies of the
                        // accumulators at every join.
                        if (left & 1) {
                            visit(recs[0]);
                            recs += 1;
                        }
                        if (left & 2) {
                            const rec_v2 w0 = recs[0], w1 = recs[1];
                            visit(w0);
                            visit(w1);
                        }
                    }
                }
                if constexpr (kProbe == 4)
                    pc[13] += any ? 1 : 0;
            };
            // one row per step (register path, kIssue experiments, !kMulti): the row of `sg` lies
            // in buffer `buf`; the hit words are renewed where a block of 64 segments starts
            auto walk = [&](int sg, int buf) {
                if ((sg & 63) == 0)
                    block_hits(sg);
                walk_row(sg, reinterpret_cast<const char *>(s_row + kStagePad + buf * rowspan + rlo + lane));
            };
            (void)walk;
            // Software pipeline over the segments.  Segment j lives in register set j % D;
            // its loads are issued D steps before its row is written to LDS buffer j % 2
            // (one step before it is walked).  Every step issues exactly R loads (the
            // segment index is clamped, a surplus row is loaded and dropped), so the number
            // of loads in flight behind the row about to be stored is a compile-time
            // constant and the wait before the store is `s_waitcnt vmcnt((D-1)*R)`.
            auto run = [&](auto Dc, auto Rc) {
                constexpr int D = decltype(Dc)::value, R = decltype(Rc)::value;
                static_assert(D == 2, "two register sets, two LDS buffers");
                load_row(0, Rc, ring);
                load_row(min(1, nseg - 1), Rc, ring + R);
                store_row(0, Rc, ring, Dc);
                __syncthreads();
                // Two steps per trip so that register sets and LDS buffers are compile-time
                // names, and NO exit inside the trip: the structurised CFG routes an exit
                // through the back edge, which leaves a static path on which the header is
                // entered with the youngest loads pending -- the compiler then drains the
                // queue (vmcnt(0)) at the top of every trip.  The last one or two segments
                // are walked after the loop.
                int sg = 0;
                for (; sg + 2 < nseg; sg += 2) {
                    load_row(sg + 2, Rc, ring);
                    walk(sg, 0);
                    store_row(1, Rc, ring + R, Dc);
                    __syncthreads();
                    load_row(min(sg + 3, nseg - 1), Rc, ring + R);
                    walk(sg + 1, 1);
                    store_row(0, Rc, ring, Dc);
                    __syncthreads();
                }
                walk(sg, 0);
                if (sg + 1 < nseg) {
                    store_row(1, Rc, ring + R, std::integral_constant<int, 1>());
                    __syncthreads();
                    walk(sg + 1, 1);
                }
            };
            // (a ring of 4 single-register sets for rows of <= 512 samples was measured:
            // it spills at the 64-VGPR budget of 8 waves/SIMD and runs 30 % slower)
            if (kDma) {
                // the row of segment sg+1 is requested by one wavefront (they take turns)
                // while sg is walked, and has landed before the barrier that ends the step.
                // (Three buffers and a request two steps ahead measured slower, 1.22 vs 1.14 ms
                // at C2: 48 KB of LDS leave three workgroups per CU.)
                if constexpr (kIssue == 1) {
                    // the turn-taking requester with its next descriptor fetched a turn ahead
                    unsigned long long dn = s_desc[min(nseg - 1, wave == 0 ? NW : wave)];
                    if (wave == 0)
                        dma_row(0, 0);
                    __builtin_amdgcn_s_waitcnt(0x0f70);
                    __syncthreads();
                    for (int sg = 0; sg < nseg; sg++) {
                        if (sg + 1 < nseg && wave == ((sg + 1) & (NW - 1))) {
                            dma_desc(dn, bufoff((sg + 1) & 1), std::false_type(), 0, 0);
                            dn = s_desc[min(nseg - 1, sg + 1 + NW)];
                        }
                        walk(sg, sg & 1);
                        __builtin_amdgcn_s_waitcnt(0x0f70);
                        __syncthreads();
                    }
                    continue;
                }
                if constexpr (kIssue == 2) {
                    // every wavefront requests its own slices of the row (8 slices of 128 samples
                    // over NW wavefronts) from a descriptor it fetched one step ahead
                    constexpr int kPer = (8 + NW - 1) / NW;
                    unsigned long long dn = s_desc[min(nseg - 1, 1)];
                    dma_desc(s_desc[0], 0, std::true_type(), wave * kPer, wave * kPer + kPer);
                    __builtin_amdgcn_s_waitcnt(0x0f70);
                    __syncthreads();
                    for (int sg = 0; sg < nseg; sg++) {
                        const unsigned long long dcur = dn;
                        dn = s_desc[min(nseg - 1, sg + 2)];
                        if (sg + 1 < nseg)
                            dma_desc(dcur, bufoff((sg + 1) & 1), std::true_type(), wave * kPer, wave * kPer + kPer);
                        walk(sg, sg & 1);
                        __builtin_amdgcn_s_waitcnt(0x0f70);
                        __syncthreads();
                    }
                    continue;
                }
                if constexpr (!kMulti) {
                    // (the two buffers take turns: `cur8` is the byte offset of the one being
                    // walked, cur8 ^ flip8 the other's, carried instead of formed per segment)
                    const unsigned flip8 = (unsigned)rowspan * 8u;
                    const char *const lane_row = reinterpret_cast<const char *>(s_row + kStagePad + rlo + lane);
                    unsigned cur8 = 0;
                    // the next segment this wavefront requests (segment g: wavefront g mod NW)
                    int mine = wave == 0 ? NW : wave;
                    unsigned long long ta = tick();
                    if (wave == 0)
                        dma_row(0, 0);
                    __builtin_amdgcn_s_waitcnt(0x0f70);           // vmcnt(0)
                    __syncthreads();
                    if constexpr (kProbe == 4) {
                        const unsigned long long tb = tick();
                        pc[8] += tb - ta;
                        ta = tb;
                    }
                    for (int sg = 0; sg < nseg; sg++, cur8 ^= flip8) {
                        if (mine == sg + 1) {
                            if (mine < nseg)
                                dma_row(mine, cur8 ^ flip8, ta);
                            mine += NW;
                        }
                        if constexpr (kProbe == 4) {
                            const unsigned long long tb = tick();
                            // (4: the wavefront whose turn it was to request the row; 18: the
                            // others, i.e. the cost of the stamp itself right after a barrier release)
                            if (sg + 1 < nseg && wave == ((sg + 1) & (NW - 1))) {
                                pc[4] += tb - ta;
                                pc[19] += 1;
                            } else {
                                pc[18] += tb - ta;
                            }
                            ta = tb;
                            const unsigned long long f0 = pc[3];
                            if ((sg & 63) == 0)
                                block_hits(sg);
                            walk_row(sg, lane_row + cur8);
                            // (every LDS value of the walk has been consumed by its FMA: lgkmcnt(0))
                            const unsigned long long tc = tick();
                            pc[5] += (tc - ta) - (pc[3] - f0);
                            __builtin_amdgcn_s_waitcnt(0x0f70);
                            const unsigned long long td = tick();
                            pc[6] += td - tc;
                            __syncthreads();
                            ta = tick();
                            pc[7] += ta - td;
                            pc[10] += 1;
                            pc[21] += 1;
                            continue;
                        }
                        if ((sg & 63) == 0)
                            block_hits(sg);
                        // (kFold: the buffer's offset is in the records; cur8 serves the request)
                        walk_row(sg, kFold ? lane_row : lane_row + cur8);
                        __builtin_amdgcn_s_waitcnt(0x0f70);       // the row of sg+1 has landed
                        __syncthreads();
                    }
                    continue;
                }
                // A step stages and walks the segments [sg, se): at most nrow of them, fewer at
                // the end of the batch and before a multiple of 64 (find_hits serves 64 segments
                // at a time, so a step never straddles one and the hit words are renewed at the
                // start of a step).  Its rows lie in the slots half * nrow + (segment - sg), the
                // two halves of the slots taking turns; the rows of the next step [se, sn) are
                // requested into the other half while this one is walked, segment g by wavefront
                // g mod NW, so no wavefront requests two rows in a row.  One wait and one barrier
                // end a step; with nrow == 1 this is one row per step in two buffers.
                // Carried from step to step instead of formed anew: `cur8`, the byte offset of the
                // half being walked (cur8 ^ flip8 is the other; a segment's slot lies pitch8 bytes
                // after the one before it), `hits_from`, the first segment the hit words do not
                // serve yet, and, where steps can straddle at all, `bend`, the end of the block of
                // 64 segments that holds `se`.  They cannot with nrow = 1 or 2 (kRows <= 2): the
                // steps of a batch start at multiples of nrow, and 64 is one, so a step's end is
                // one add and one min.
                constexpr bool kAligned = kRows <= 2;
                const unsigned pitch8 = (unsigned)pitch * 8u, flip8 = (unsigned)nrow * pitch8;
                const char *const lane_row = reinterpret_cast<const char *>(s_row + kStagePad + rlo + lane);
                // `mine`: the next segment this wavefront requests.  The steps are requested in
                // order and hold at most NW segments, so on entry it is the one segment at or
                // after s0 that is this wavefront's, and the test is one compare.
                int mine = wave;
                auto request = [&](int s0, int s1, unsigned boff0, unsigned long long tref) {
                    const bool ask = mine < s1;
                    if (ask) {
                        dma_row(mine, boff0 + (unsigned)(mine - s0) * pitch8, tref);
                        mine += NW;
                    }
                    return ask;
                };
                unsigned long long ta = tick();
                int bend = kAligned ? nseg : min(64, nseg);
                int sg = 0, se = min(nrow, bend), hits_from = 0;
                unsigned cur8 = 0;
                // (a step holds at least one segment: no test before the first)
                auto walk_step = [&]() {
                    if (sg == hits_from) {
                        block_hits(sg);
                        hits_from += 64;
                    }
                    int g = sg;
                    if constexpr (kFold) {
                        // (the slot's offset is in the records of the segment)
                        do {
                            walk_row(g, lane_row);
                        } while (++g < se);
                    } else {
                        const char *rp = lane_row + cur8;
                        do {
                            walk_row(g, rp);
                            rp += pitch8;
                        } while (++g < se);
                    }
                };
                request(0, se, 0, 0);
                __builtin_amdgcn_s_waitcnt(0x0f70);           // vmcnt(0)
                __syncthreads();
                if constexpr (kProbe == 4) {
                    const unsigned long long tb = tick();
                    pc[8] += tb - ta;
                    ta = tb;
                }
                do {                                      // nseg > 0
                    if constexpr (!kAligned) {
                        if (se == bend)
                            bend = min(bend + 64, nseg);
                    }
                    const int sn = min(se + nrow, bend);
                    const bool asked = request(se, sn, cur8 ^ flip8, ta);
                    if constexpr (kProbe == 4) {
                        const unsigned long long tb = tick();
                        // (4: the wavefronts whose turn it was to request a row; 18: the others,
                        // i.e. the cost of the stamp itself right after a barrier release)
                        if (asked) {
                            pc[4] += tb - ta;
                            pc[19] += 1;
                        } else {
                            pc[18] += tb - ta;
                        }
                        ta = tb;
                        const unsigned long long f0 = pc[3];
                        walk_step();
                        // (every LDS value of the walk has been consumed by its FMA: lgkmcnt(0))
                        const unsigned long long tc = tick();
                        pc[5] += (tc - ta) - (pc[3] - f0);
                        __builtin_amdgcn_s_waitcnt(0x0f70);
                        const unsigned long long td = tick();
                        pc[6] += td - tc;
                        __syncthreads();
                        ta = tick();
                        pc[7] += ta - td;
                        pc[10] += 1;
                        pc[21] += (unsigned long long)(se - sg);
                    } else {
                        (void)asked;
                        walk_step();
                        __builtin_amdgcn_s_waitcnt(0x0f70);   // the rows of [se, sn) have landed
                        __syncthreads();
                    }
                    sg = se;
                    se = sn;
                    cur8 ^= flip8;
                } while (sg < nseg);
            } else if (nseg > 0) {
                run(std::integral_constant<int, 2>(), std::integral_constant<int, kRowRegs>());
            }
        }
    }

    const unsigned long long t_out = tick();
#pragma unroll
    for (int u = 0; u < S; u++) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int j = rlo + u * kSub + c * 64 + lane;
            if (j < tlen)
                dst[j] = acc[u][c];
        }
    }
    if constexpr (kProbe == 4) {
        const unsigned long long t_end = tick();
        pc[14] += t_end - t_out;
        pc[9] = t_end - t_birth;
        pc[15] = (unsigned long long)__builtin_amdgcn_s_memrealtime() - real_birth;
        if (lane == 0 && a.probe)
            for (int i = 0; i < 22; i++)
                atomicAdd(&a.probe[(int64_t)layer * 24 + i], pc[i]);
    }
}

// ---------------------------------------------------------------------------
// 3a''. Resident-profile gather (constant-step grid), for layers whose profiles are narrow:
// the WHOLE phase-major block of a table cell (osamp rows of a few tens of samples,
// <= res_cap doubles) is copied into LDS once per (workgroup, isotope, cell), and then
// every lane owns ONE output sample and walks, in position order, the records whose window
// reaches its wavefront's 64 samples: one 16-byte broadcast read of the record, one
// `ds_read_b64` of row[phi][sample + q] and one fma per (record, 64 samples), with a
// per-lane window predicate that redirects outside lanes to a zero slot.
// With ~20-sample rows a record costs 64 lanes of work instead of the 256 (staged) or 512
// (global) of the kernels above, and there are no per-phase segments to synchronise on.
// The terms of a sample are added in (isotope, position) order -- the order of the global
// gather -- whatever the tiling.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kResThreads) void k_ext_resident(LblArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    struct __align__(16) Rec {
        double k;
        int off;                  // LDS byte offset of tile sample 0 in the record's phase row
        unsigned win;             // lo | length << 16 (tile coordinates)
    };
    double *s_prof = reinterpret_cast<double *>(smem);                   // [res_cap] + zero slot
    const int zslot = a.res_cap;
    Rec *s_rec = reinterpret_cast<Rec *>(s_prof + a.res_cap + 2);        // [kResThreads]
    int *s_cell = reinterpret_cast<int *>(s_rec + kResThreads);          // [kResThreads]
    int *s_part = s_cell + kResThreads;                                  // [kResWaves]

    int tile, layer;
    decode_block(a, tile, layer);
    if (layer < 0 || !a.ls_resident[layer])
        return;
    const int row = blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const int64_t t0 = a.wbegin + (int64_t)tile * kResTile;
    const int64_t tend = min(t0 + kResTile, a.wbegin + a.wcount);
    const int tlen = (int)(tend - t0);
    const double kthresh =
        a.ethresh * __longlong_as_double((long long)a.kmax_bits[(int64_t)layer * a.nrows + row]);
    const int64_t recbase = (int64_t)layer * a.ngroups;
    const int osamp = a.osamp;
    const int ofactor = a.ls_ofactor[layer];

    double acc[kResStrips];
#pragma unroll
    for (int u = 0; u < kResStrips; u++)
        acc[u] = 0.0;
    if (tid == 0)
        s_prof[zslot] = 0.0;

    for (int iso = 0; iso < a.niso; iso++) {
        const int iext = a.isoiext[iso];
        if (iext < 0 || (a.add ? 0 : iext) != row)
            continue;
        const int64_t li = (int64_t)layer * a.niso + iso;
        const double dens = a.li_dens[li];
        int64_t reach = a.li_hmax[li];
        if (a.cutoff > 0.0)
            reach = min(reach, (int64_t)(a.cutoff / a.ownstep) + 2 * (int64_t)ofactor + 2);
        reach += osamp + ofactor;
        // candidates: groups at fine positions [t0*osamp - reach, (tend-1)*osamp + reach],
        // bracketed through the per-sample index of the position-sorted list
        const int64_t rs = reach / osamp + 1;
        const int32_t *gs = a.gs_start + (int64_t)iso * (a.nwave + 1);
        const int64_t g0 = gs[max((int64_t)0, t0 - rs)];
        const int64_t g1 = gs[min((int64_t)a.nwave, tend + rs)];

        for (int64_t gb = g0; gb < g1; gb += kResThreads) {
            const int nrec = (int)min((int64_t)kResThreads, g1 - gb);
            __syncthreads();               // the previous walk has finished with s_rec / s_prof
            {
                double k = 0.0;
                unsigned win = 0;
                int off = 0, cell = -1;
                if (tid < nrec) {
                    const int64_t idx = recbase + gb + tid;
                    k = a.rec_k[idx];
                    const int ulo = a.rec_ulo[idx], uhi = a.rec_uhi[idx];
                    const int lo = (int)(max((int64_t)ulo, t0) - t0);
                    const int hi = (int)(min((int64_t)uhi, tend) - t0);
                    if (!(k < kthresh) && lo < hi) {
                        if (a.add)
                            k *= dens;
                        cell = a.rec_cell[idx];
                        win = (unsigned)lo | ((unsigned)(hi - lo) << 16);
                        // tile sample j reads s_prof[phi*stride + (j + t0 + q)]
                        off = 8 * (a.rec_phi[idx] * a.pm_stride[cell] + (int)(a.rec_q[idx] + t0));
                    } else {
                        k = 0.0;
                    }
                }
                s_rec[tid].k = k;
                s_rec[tid].off = off;
                s_rec[tid].win = win;
                s_cell[tid] = cell;
            }
            // the cells of a batch, in ascending order (the Doppler index grows with position)
            int cur = -1;
            for (;;) {
                __syncthreads();
                int c = s_cell[tid];
                c = c > cur ? c : INT_MAX;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1)
                    c = min(c, __shfl_xor(c, d));
                if (lane == 0)
                    s_part[wave] = c;
                __syncthreads();
                c = INT_MAX;
                for (int w = 0; w < kResWaves; w++)
                    c = min(c, s_part[w]);
                if (c == INT_MAX)
                    break;
                cur = c;
                // ---- the cell's phase-major block -> LDS ----
                {
                    const int n = a.pm_stride[cur] * osamp;
                    const double *src = a.pm + a.pm_base[cur];
                    for (int i = tid; i < n; i += kResThreads)
                        s_prof[i] = src[i];
                }
                __syncthreads();
                // ---- every wavefront walks the records that reach its strips ----
                const double2 *recs = reinterpret_cast<const double2 *>(s_rec);
#pragma unroll
                for (int u = 0; u < kResStrips; u++) {
                    const int slo = (wave + u * kResWaves) * 64;
                    if (slo >= tlen)
                        continue;
                    int first = INT_MAX, last = -1;
                    for (int b = 0; b < nrec; b += 64) {
                        const int e = b + lane;            // < kResThreads
                        const unsigned w = s_rec[e].win;
                        const int wlo = (int)(w & 0xffff);
                        const bool hit = s_cell[e] == cur && wlo < slo + 64 &&
                                         wlo + (int)(w >> 16) > slo;
                        const unsigned long long m = __ballot(hit);
                        if (m) {
                            first = min(first, b + (int)__builtin_ctzll(m));
                            last = max(last, b + 63 - (int)__builtin_clzll(m));
                        }
                    }
                    first = __builtin_amdgcn_readfirstlane(first);
                    last = __builtin_amdgcn_readfirstlane(last);
                    const unsigned j = (unsigned)(slo + lane);
                    typedef __attribute__((address_space(3))) const double lds_double;
                    // LDS byte addresses: the lane's sample in row 0, and the zero slot
                    const unsigned prof0 = (unsigned)(uintptr_t)(
                        (__attribute__((address_space(3))) const char *)s_prof);
                    const unsigned j8 = prof0 + j * 8u, z8 = prof0 + (unsigned)zslot * 8u;
                    double sum = acc[u];
#pragma unroll 4
                    for (int r = first; r <= last; r++) {
                        const double2 raw = recs[r];
                        const unsigned w = (unsigned)__double2hiint(raw.y);
                        const bool in = j - (w & 0xffffu) < (w >> 16);
                        const unsigned at = in ? j8 + (unsigned)__double2loint(raw.y) : z8;
                        sum = fma(raw.x, *(lds_double *)(uintptr_t)at, sum);
                    }
                    acc[u] = sum;
                }
            }
        }
    }

    double *dst = a.ext + ((int64_t)layer * a.nrows + row) * a.wcount + (t0 - a.wbegin);
#pragma unroll
    for (int u = 0; u < kResStrips; u++) {
        const int j = (wave + u * kResWaves) * 64 + lane;
        if (j < tlen)
            dst[j] = acc[u];
    }
}

#ifdef PB_EXPERIMENTS   // gather mode 4 (4x slower than the staged kernel)
// ---------------------------------------------------------------------------
// 3s. Scatter kernel (constant-step grid): ONE wavefront owns a tile of T output samples
// held in LDS and walks, in (isotope, position) order, the records whose window reaches the
// tile.  Per record and 64 samples: one coalesced `buffer_load_dwordx2` straight from the
// phase-major table (the window is the buffer, lanes past its end read 0), one v_mul_f64,
// one `ds_add_f64` into the tile -- products and sums rounded separately like the
// reference's `ktmp[j] += k * profile[...]`.  No staging, no phase sorting, no workgroup
// barrier; the table traffic is exactly the window lengths.  Record fields are wave-uniform
// and arrive by scalar loads.  The tile belongs to one wavefront and LDS executes a
// wavefront's operations in order, so every sample is summed in record order whatever the
// tiling: results are bitwise reproducible and shards concatenate exactly.
// ---------------------------------------------------------------------------
constexpr int kScatterPad = 64;       // lanes past a window's end add zeros there

// The walk of one tile with C chunks (64 samples each) per record in flight.
template <int C>
__device__ inline void scatter_walk(const LblArgs &a, double *s_tile, int layer, int row,
                                    int64_t t0, int64_t tend, double kthresh)
{
    typedef int v2i __attribute__((ext_vector_type(2)));
    typedef int v4i __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x;
    const int osamp = a.osamp;
    const int ofactor = a.ls_ofactor[layer];
    const Rec32 *recs = a.rec32 + (int64_t)layer * a.ngroups;

    for (int iso = 0; iso < a.niso; iso++) {
        const int iext = a.isoiext[iso];
        if (iext < 0 || (a.add ? 0 : iext) != row)
            continue;
        const int64_t li = (int64_t)layer * a.niso + iso;
        const double dens = a.add ? a.li_dens[li] : 1.0;
        int64_t reach = a.li_hmax[li];
        if (a.cutoff > 0.0)
            reach = min(reach, (int64_t)(a.cutoff / a.ownstep) + 2 * (int64_t)ofactor + 2);
        reach += osamp + ofactor;
        const int64_t rs = reach / osamp + 1;
        const int32_t *gs = a.gs_start + (int64_t)iso * (a.nwave + 1);
        const int g0 = gs[max((int64_t)0, t0 - rs)];
        const int g1 = gs[min((int64_t)a.nwave, tend + rs)];

        // 64 records per batch, one per lane; the next batch is requested before this one
        // is walked
        v4i w0 = {0, 0, 0, 0}, w1 = {0, 0, 0, 0};
        auto fetch = [&](int g) {
            const v4i *p = reinterpret_cast<const v4i *>(recs + min(g + lane, g1 - 1));
            w0 = p[0];
            w1 = p[1];
        };
        if (g0 < g1)
            fetch(g0);
        for (int gb = g0; gb < g1; gb += 64) {
            const double kk = __hiloint2double(w0.y, w0.x);
            const long long off = ((long long)w0.w << 32) | (unsigned)w0.z;
            const int lo = max(w1.x, (int)t0), hi = min(w1.y, (int)tend);
            const bool ok = gb + lane < g1 && !(kk < kthresh) && lo < hi;
            const double b_k = kk * dens;
            const long long b_src = off + lo;
            const int b_lo = lo - (int)t0, b_n = hi - lo;
            unsigned long long live = __ballot(ok);
            if (gb + 64 < g1)
                fetch(gb + 64);

            // the live records, two in flight: the C loads of the next one are issued before
            // the current one is multiplied and added
            struct Cur {
                int dst, nch;
                double k;
            };
            auto start = [&](double (&v)[C], Cur &c) {
                const int sl = (int)__builtin_ctzll(live);
                live &= live - 1;
                c.k = bcast(b_k, sl);
                const int s_lo = __builtin_amdgcn_readlane((int)b_src, sl);
                const int s_hi = __builtin_amdgcn_readlane((int)(b_src >> 32), sl);
                const int n = __builtin_amdgcn_readlane(b_n, sl);
                c.dst = __builtin_amdgcn_readlane(b_lo, sl);
                c.nch = (n + 63) >> 6;
                const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
                    (void *)(a.pm + (((long long)s_hi << 32) | (unsigned)s_lo)), 0, n * 8,
                    0x00020000);
#pragma unroll
                for (int q = 0; q < C; q++) {
                    const v2i w = __builtin_amdgcn_raw_buffer_load_b64(rsrc, lane * 8, q * 512, 0);
                    v[q] = __hiloint2double(w.y, w.x);
                }
            };
            auto finish = [&](const double (&v)[C], const Cur &c) {
                double *dst = s_tile + c.dst + lane;
#pragma unroll
                for (int q = 0; q < C; q++)
                    if (q < c.nch)
                        __hip_atomic_fetch_add(dst + q * 64, c.k * v[q], __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
            };
            double va[C], vb[C];
            Cur ca, cb;
            if (!live)
                continue;
            start(va, ca);
            for (;;) {
                if (!live) {
                    finish(va, ca);
                    break;
                }
                start(vb, cb);
                finish(va, ca);
                if (!live) {
                    finish(vb, cb);
                    break;
                }
                start(va, ca);
                finish(vb, cb);
            }
        }
    }
}

template <int T>
__global__ __launch_bounds__(64) void k_ext_scatter(LblArgs a)
{
    __shared__ double s_tile[T + kScatterPad];
    int tile, layer;
    decode_block(a, tile, layer);
    if (layer < 0)
        return;
    const int row = blockIdx.y;
    const int lane = threadIdx.x;
    const int64_t t0 = a.wbegin + (int64_t)tile * T;
    const int64_t tend = min(t0 + T, a.wbegin + a.wcount);
    const int tlen = (int)(tend - t0);
    const double kthresh =
        a.ethresh * __longlong_as_double((long long)a.kmax_bits[(int64_t)layer * a.nrows + row]);
    for (int i = lane; i < T + kScatterPad; i += 64)
        s_tile[i] = 0.0;
    // chunks per record: the longest phase row this layer can select
    const int rowmax = a.ls_block[layer] / a.osamp;
    const int chunks = (min(rowmax, T) + 63) >> 6;
    if (chunks <= 4)
        scatter_walk<4>(a, s_tile, layer, row, t0, tend, kthresh);
    else if (chunks <= 6)
        scatter_walk<6>(a, s_tile, layer, row, t0, tend, kthresh);
    else if (chunks <= 8)
        scatter_walk<8>(a, s_tile, layer, row, t0, tend, kthresh);
    else if (chunks <= 12)
        scatter_walk<12>(a, s_tile, layer, row, t0, tend, kthresh);
    else if (chunks <= 16)
        scatter_walk<16>(a, s_tile, layer, row, t0, tend, kthresh);
    else
        scatter_walk<32>(a, s_tile, layer, row, t0, tend, kthresh);
    __builtin_amdgcn_s_waitcnt(0);     // the tile is complete (same wavefront: in order)
    double *out = a.ext + ((int64_t)layer * a.nrows + row) * a.wcount + (t0 - a.wbegin);
    for (int i = lane; i < tlen; i += 64)
        out[i] = s_tile[i];
}

#endif  // PB_EXPERIMENTS

// ext += part[0] + part[1] + ... in that order (the phase splits of a small staged launch).
// skip[layer] != 0: a layer another kernel computed whole (the resident-profile kernel): the
// staged kernel wrote NO partial sums for it, its planes hold whatever an earlier call left there
// (found by tools/fuzz_r4.py: a plan used in `staged` mode and then in automatic mode with resident
// layers added the earlier call's pieces to the resident kernel's result; on a fresh plan the
// planes are fresh zero pages, which is why no test saw it).
__global__ __launch_bounds__(kBlock) void k_combine_parts(double *ext, const double *part,
                                                         int nparts, int64_t n,
                                                         const int32_t *skip, int64_t per_layer)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    if (skip && skip[i / per_layer])
        return;
    double v = ext[i];
    for (int p = 0; p < nparts; p++)
        v += part[(int64_t)p * n + i];
    ext[i] = v;
}

// the same with a per-tile number of pieces (LblArgs::tsplit): sample w of a row belongs to tile
// w / tile and has tsplit[tile] - 1 partial planes
__global__ __launch_bounds__(kBlock) void k_combine_tile_parts(double *ext, const double *part,
                                                              const int32_t *tsplit, int tile,
                                                              int64_t wcount, int64_t n,
                                                              const int32_t *skip, int64_t per_layer)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const int np = tsplit[(i % wcount) / tile] - 1;
    if (np <= 0 || (skip && skip[i / per_layer]))
        return;
    double v = ext[i];
    for (int p = 0; p < np; p++)
        v += part[(int64_t)p * n + i];
    ext[i] = v;
}

// the same with a per-layer number of pieces: grid.y = layer, layers in one piece are skipped
__global__ __launch_bounds__(kBlock) void k_combine_layer_parts(double *ext, const double *part,
                                                               const int32_t *lsplit,
                                                               int64_t per_layer, int64_t n,
                                                               const int32_t *skip)
{
    const int layer = blockIdx.y;
    const int nparts = lsplit[layer] - 1;
    if (nparts <= 0 || (skip && skip[layer]))
        return;
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= per_layer)
        return;
    const int64_t i = (int64_t)layer * per_layer + j;
    double v = ext[i];
    for (int p = 0; p < nparts; p++)
        v += part[(int64_t)p * n + i];
    ext[i] = v;
}

}  // namespace

namespace pbx {

GatherKernel staged_kernel(int S, bool dma, int rows)
{
    constexpr int R = kStageRowsMax;
    if (dma && rows > 1)
        return S == 4   ? k_ext_staged<kStagedWaves, 4, true, 0, 0, R>
               : S == 2 ? k_ext_staged<kStagedWaves, 2, true, 0, 0, R>
                        : k_ext_staged<kStagedWaves, 1, true, 0, 0, R>;
    return dma ? (S == 4   ? k_ext_staged<kStagedWaves, 4, true>
                  : S == 2 ? k_ext_staged<kStagedWaves, 2, true>
                           : k_ext_staged<kStagedWaves, 1, true>)
               : (S == 4   ? k_ext_staged<kStagedWaves, 4, false>
                  : S == 2 ? k_ext_staged<kStagedWaves, 2, false>
                           : k_ext_staged<kStagedWaves, 1, false>);
}

// a kernel that asks for more than 64 KiB of dynamic LDS has to say so first
int allow_lds(const void *kern, size_t lds)
{
    if (lds > 64 * 1024)
        PB_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return PB_OK;
}

#ifdef PB_EXPERIMENTS
// the measured dead ends (`make EXPERIMENTS=1`) that launch kernels of this file: the scatter
// gather, the round gather (its k_combine_parts pass) and the probes of the staged kernel
int exp_launch_scatter(LblArgs &a, const Tuning &tn, hipStream_t s)
{
    const int T = tn.scatter_t;
    a.ntiles = pb::div_up(a.wcount, T);
    dim3 grid((unsigned)(8 * a.ntiles * ((a.nlayers + 7) / 8)), a.nrows);
    if (T == 2048)
        k_ext_scatter<2048><<<grid, 64, 0, s>>>(a);
    else if (T == 1024)
        k_ext_scatter<1024><<<grid, 64, 0, s>>>(a);
    else
        k_ext_scatter<512><<<grid, 64, 0, s>>>(a);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int exp_launch_rounds(pb_lbl *p, LblArgs &a, const GatherPlan &g, const Tuning &tn,
                      hipStream_t s)
{
    const pb_voigt *v = p->voigt;
    const pb_lines *l = p->lines;
    const int nlayers = a.nlayers;
    const int64_t wbegin = a.wbegin, wcount = a.wcount;
    // geometry: 16 wavefronts x 2 spans of 256 samples (tile 8192, two LDS buffers of 8192
    // samples, one workgroup per CU) or 8 x 2 (tile 4096, buffers of 4096, two per CU)
    const int geom = tn.rounds_geom;
    int T = 0;
    rounds_geometry(geom, &T, &a.rbuf);
    a.rtile = T;
    a.ntiles = pb::div_up(wcount, T);
    int rsplit = (int)std::min<int64_t>(
        8, pb::div_up((int64_t)(g.per_phase >= 64.0 ? 4000 : 1000),
                      std::max<int64_t>(1, (int64_t)a.ntiles * nlayers)));
    if (tn.stage_split)
        rsplit = tn.stage_split;
    rsplit = cap_split_to_planes(rsplit, plane_bytes(a));
    a.nsplit = rsplit;
    if (int rc = ensure_part(p, a, rsplit, s))
        return rc;
    // the largest distance from which a group can reach a tile, over all layers
    const int64_t reachmax = group_reach(v, a.cutoff, a.ownstep) + 2 * (int64_t)v->osamp;
    a.reachmax = reachmax;
    const int nunits = a.ntiles * rsplit;
    if (p->cap_key[0] != wbegin || p->cap_key[1] != wcount || p->cap_key[2] != T ||
        p->cap_key[3] != rsplit) {
        // capacity of every unit: the groups (any isotope) within reach of its tile
        std::vector<int64_t> cap((size_t)nunits + 1, 0);
        for (int t = 0; t < a.ntiles; t++) {
            const int64_t t0 = wbegin + (int64_t)t * T;
            const int64_t tend = std::min(t0 + T, wbegin + wcount);
            int64_t n = groups_in_reach(l, p->niso, t0 * v->osamp - reachmax,
                                        (tend - 1) * v->osamp + reachmax);
            n = (n + 3) & ~(int64_t)3;
            for (int z = 0; z < rsplit; z++)
                cap[(size_t)t * rsplit + z + 1] = n;
        }
        for (int u = 0; u < nunits; u++)
            cap[(size_t)u + 1] += cap[(size_t)u];
        PB_HIP(hipStreamSynchronize(s));       // an earlier call may still read the lists
        if (int rc = ensure_bytes((void **)&p->unit_cap, &p->unit_cap_bytes, cap.size() * 8, s,
                                  false, nullptr))
            return rc;
        PB_HIP(hipMemcpy(p->unit_cap, cap.data(), cap.size() * 8, hipMemcpyHostToDevice));
        p->cap_key[0] = wbegin;
        p->cap_key[1] = wcount;
        p->cap_key[2] = T;
        p->cap_key[3] = rsplit;
        p->cap_key[4] = cap.back();
    }
    const size_t nent = (size_t)nlayers * a.nrows * (size_t)p->cap_key[4] + 4;
    if (nent > p->vrec_alloc) {
        // the three lists grow together (vrec_alloc entries each)
        size_t b0 = 0, b1 = 0, b2 = 0;
        p->vrec_alloc = 0;
        PB_HIP(hipStreamSynchronize(s));
        int rc = ensure_bytes((void **)&p->vrec, &b0, nent * 16, s, false, "visit records");
        if (rc == PB_OK)
            rc = ensure_bytes((void **)&p->vseg, &b1, nent * 16, s, false, "visit records");
        if (rc == PB_OK)
            rc = ensure_bytes((void **)&p->vrnd, &b2, nent * 4, s, false, "visit records");
        if (rc)
            return rc;
        p->vrec_alloc = nent;
    }
    const size_t nhdr = (size_t)nlayers * a.nrows * nunits;
    if (int rc = ensure_bytes((void **)&p->uhdr, &p->uhdr_bytes, nhdr * 16, s, true, nullptr))
        return rc;
    a.unit_cap = p->unit_cap;
    a.vrec = p->vrec;
    a.vseg = p->vseg;
    a.vrnd = p->vrnd;
    a.uhdr = p->uhdr;
    if (int rc = rounds_launch(a, geom, s))
        return rc;
    if (rsplit > 1) {
        const int64_t n = (int64_t)nlayers * a.nrows * wcount;
        k_combine_parts<<<(unsigned)pb::div_up(n, kBlock), kBlock, 0, s>>>(
            a.ext, p->part, rsplit - 1, n, nullptr, (int64_t)a.nrows * wcount);
    }
    PB_LAUNCH_CHECK();
    return PB_OK;
}

// PB_STAGE_PROBE: instrumented instances of the staged kernel in place of `kern`
static int exp_stage_probe_begin(LblArgs &a, const GatherPlan &g, const Tuning &tn,
                                 GatherKernel *kern, hipStream_t s)
{
    const int e = tn.stage_probe;
    if (g.S != 2 || !g.dma)
        return PB_OK;
    if (e >= 1 && e <= 3)                                 // 1, 2: timing probes, wrong sums
        *kern = e == 1   ? k_ext_staged<kStagedWaves, 2, true, 1>
                : e == 2 ? k_ext_staged<kStagedWaves, 2, true, 2>
                         : k_ext_staged<kStagedWaves, 2, true, 3>;
    if (e >= 11 && e <= 12)                               // 11, 12: who requests the row DMA
        *kern = e == 11 ? k_ext_staged<kStagedWaves, 2, true, 0, 1>
                        : k_ext_staged<kStagedWaves, 2, true, 0, 2>;
    if (e == 4) {                                         // the cycle account (valid sums)
        *kern = a.rows_cap > 1 ? k_ext_staged<kStagedWaves, 2, true, 4, 0, kStageRowsMax>
                               : k_ext_staged<kStagedWaves, 2, true, 4>;
        PB_HIP(hipMalloc(&a.probe, (size_t)a.nlayers * 24 * 8));
        PB_HIP(hipMemsetAsync(a.probe, 0, (size_t)a.nlayers * 24 * 8, s));
    }
    return PB_OK;
}

static int exp_stage_probe_end(LblArgs &a, hipStream_t s)
{
    if (!a.probe)
        return PB_OK;
    // one line per layer on stderr: layer, rowmax of its first isotope, then the 15 sums
    std::vector<unsigned long long> h((size_t)a.nlayers * 24);
    PB_HIP(hipMemcpyAsync(h.data(), a.probe, h.size() * 8, hipMemcpyDeviceToHost, s));
    std::vector<int32_t> rowmax((size_t)a.nlayers * a.niso);
    PB_HIP(hipMemcpyAsync(rowmax.data(), a.li_rowmax, rowmax.size() * 4,
                          hipMemcpyDeviceToHost, s));
    PB_HIP(hipStreamSynchronize(s));
    (void)hipFree(a.probe);
    a.probe = nullptr;
    for (int layer = 0; layer < a.nlayers; layer++) {
        fprintf(stderr, "STAGE_PROBE layer %d rowmax %d :", layer,
                rowmax[(size_t)layer * a.niso]);
        for (int i = 0; i < 22; i++)
            fprintf(stderr, " %llu", h[(size_t)layer * 24 + i]);
        fprintf(stderr, "\n");
    }
    return PB_OK;
}
#else
static inline int exp_stage_probe_begin(LblArgs &, const GatherPlan &, const Tuning &,
                                        GatherKernel *, hipStream_t) { return PB_OK; }
static inline int exp_stage_probe_end(LblArgs &, hipStream_t) { return PB_OK; }
#endif  // PB_EXPERIMENTS

// Per-tile split table of the staged kernel (LblArgs::tsplit), cached per tiling: from the
// groups within reach of every tile the tiles above 1.5 x the median count get more pieces, up
// to 8; the others keep the launch's `nsplit`.
static int tile_split_table(pb_lbl *p, const LblArgs &a, const GatherPlan &g, const Tuning &tn,
                            int nsplit, hipStream_t s)
{
    const pb_voigt *v = p->voigt;
    const pb_lines *l = p->lines;
    const int64_t wbegin = a.wbegin, wcount = a.wcount;
    const int tile = g.S * (int)kStagedSub;
    const int nt = pb::div_up(wcount, tile);
    if (p->ts_key[0] == wbegin && p->ts_key[1] == wcount && p->ts_key[2] == tile &&
        p->ts_key[3] == nsplit)
        return PB_OK;
    const int64_t reach = group_reach(v, a.cutoff, a.ownstep);
    std::vector<int64_t> cnt((size_t)nt, 0);
    for (int t = 0; t < nt; t++) {
        const int64_t t0 = wbegin + (int64_t)t * tile;
        const int64_t tend = std::min<int64_t>(t0 + tile, wbegin + wcount);
        cnt[(size_t)t] = groups_in_reach(l, p->niso, t0 * v->osamp - reach,
                                         (tend - 1) * v->osamp + reach);
    }
    std::vector<int64_t> sorted(cnt);
    std::nth_element(sorted.begin(), sorted.begin() + nt / 2, sorted.end());
    const double median = (double)std::max<int64_t>(1, sorted[(size_t)nt / 2]);
    std::vector<int32_t> ts((size_t)nt);
    int tmax = nsplit;
    if (tn.tile_debug) {
        fprintf(stderr, "tile counts (median %.0f):", median);
        for (int t = 0; t < nt; t++)
            fprintf(stderr, " %lld", (long long)cnt[(size_t)t]);
        fprintf(stderr, "\n");
    }
    // groups per (2048 samples, phase row) of a tile against the threshold that sends a
    // whole launch to the global gather: a tile below it is visit-starved in the staged
    // kernel (~300 barrier steps of one or two records: as long as a full tile) -- once
    // SOME tile is dense enough to be split, the sparse ones go to the global gather
    bool sparse = false, dense = false;
    for (int t = 0; t < nt; t++) {
        const int k = std::max(tn.tile_min, (int)std::ceil((double)cnt[(size_t)t] / (1.5 * median)));
        ts[(size_t)t] = std::max(nsplit, std::min(8, nsplit * std::max(1, k)));
        tmax = std::max(tmax, ts[(size_t)t]);
        dense = dense || ts[(size_t)t] > nsplit;
    }
    if (dense && g.packable && p->pos2ph && !tn.tile_global_off)
        for (int t = 0; t < nt; t++) {
            const double per =
                (double)cnt[(size_t)t] * 2048.0 / (double)tile / (double)v->osamp;
            if (per < p->stage_threshold) {
                ts[(size_t)t] = 0;
                sparse = true;
            }
        }
    p->ts_sparse = sparse;
    PB_HIP(hipStreamSynchronize(s));       // an earlier call may still read the table
    if (int rc = ensure_bytes((void **)&p->d_tsplit, &p->ts_bytes, (size_t)nt * 4, s, false, nullptr))
        return rc;
    PB_HIP(hipMemcpy(p->d_tsplit, ts.data(), (size_t)nt * 4, hipMemcpyHostToDevice));
    p->ts_key[0] = wbegin;
    p->ts_key[1] = wcount;
    p->ts_key[2] = tile;
    p->ts_key[3] = nsplit;
    p->ts_max = tmax;
    return PB_OK;
}

// Per-layer split tables of the staged kernel (LblArgs::unit_tab, lsplit), cached: the deepest
// `deep` layers in `deep_split` pieces, the others in `nsplit`, in dispatch order.
static int layer_split_table(pb_lbl *p, int nlayers, int nsplit, int deep, int deep_split,
                             hipStream_t s)
{
    if (p->ut_key[0] == nlayers && p->ut_key[1] == nsplit && p->ut_key[2] == deep &&
        p->ut_key[3] == deep_split)
        return PB_OK;
    std::vector<int32_t> tab, ls((size_t)nlayers);
    for (int layer = nlayers - 1; layer >= 0; layer--) {
        const int n = layer >= nlayers - deep ? deep_split : nsplit;
        ls[(size_t)layer] = n;
        for (int z = 0; z < n; z++)
            tab.push_back((layer << 8) | z);
    }
    PB_HIP(hipStreamSynchronize(s));       // an earlier call may still read the tables
    if (int rc = ensure_bytes((void **)&p->d_unit_tab, &p->ut_bytes, tab.size() * 4, s, false, nullptr))
        return rc;
    if (int rc = ensure_bytes((void **)&p->d_lsplit, &p->ls_bytes, ls.size() * 4, s, false, nullptr))
        return rc;
    PB_HIP(hipMemcpy(p->d_unit_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(p->d_lsplit, ls.data(), ls.size() * 4, hipMemcpyHostToDevice));
    p->ut_key[0] = nlayers;
    p->ut_key[1] = nsplit;
    p->ut_key[2] = deep;
    p->ut_key[3] = deep_split;
    p->ut_units = (int)tab.size();
    return PB_OK;
}

int launch_staged(pb_lbl *p, LblArgs &a, const GatherPlan &g, const Tuning &tn, hipStream_t s)
{
    const int nlayers = a.nlayers;
    const int64_t wcount = a.wcount;
    const int64_t plane = plane_bytes(a);
    int nsplit = g.nsplit;
    // Per-layer split.  A launch ends when its slowest workgroup does, and the slowest are the
    // tiles of the deepest layers (cutoff-limited windows of ~1000 samples against 200-300
    // higher up: 0.7-0.9 ms of a 0.88-ms C2 launch, profiles/r02_gather_ab.md), which the
    // dispatch order puts first.  The deepest `deep` layers are cut into more pieces than the
    // others, so that no single workgroup spans the launch.  Pieces of a tile add their sums in
    // a fixed order (k_combine_layer_parts): bitwise reproducible; against an unsplit launch
    // the association of a sample's terms differs (~1e-16).  PB_STAGE_SPLIT pins one split for
    // every layer (the exactness tests), PB_STAGE_DEEP=frac[,factor] tunes the rule.
    // Measured (profiles/r03_gather_ab.md): C3 44.1 -> 42.3 ms (-4 %), the 1e6-line list -1 %,
    // C2 +4 % (one spectrum at a time) / +3 % (pipelined): the second prologue and the combine
    // pass cost a light launch more than its tail does.  On by default only for long rows.
    int deep = 0, deep_split = nsplit;
    if (!tn.stage_split && nsplit < 8 && nlayers >= 8) {
        const double frac = tn.deep_set ? tn.deep_frac : a.nch_max > 1 ? 0.3 : 0.0;
        const int factor = tn.deep_set ? tn.deep_factor : 2;
        deep = (int)(frac * nlayers + 0.5);
        deep_split = cap_split_to_planes(std::min(8, nsplit * factor), plane, nsplit);
        if (deep <= 0 || deep_split <= nsplit)
            deep = 0, deep_split = nsplit;
    }
    // Per-tile split.  A uniform line list gives every tile the same number of records; a
    // real one has band heads (10^2-10^3 x the line density of the gaps): the few tiles under
    // a head run 10 x as long as the others and end the launch alone (the C2 grid with 8 band
    // heads per isotope at 300 x contrast: gather 1.90 ms unsplit, 1.34 ms with every tile in
    // four pieces -- profiles/r04_bands.md).  From the groups within reach of every tile (host
    // copy of the group positions, cached per tiling) the tiles above 1.5 x the median count
    // get more pieces, up to 8; the others keep the launch's.  Automatic mode only: a forced
    // mode adds the terms of a sample in one order whatever the tiling (pbhip.h).
    if (deep == 0 && a.nch_max == 1 && p->gather_mode == 0 && a.wave_cap == 0 &&
        !tn.stage_split && !tn.tile_split_off && !p->lines->h_giown.empty()) {
        if (int rc = tile_split_table(p, a, g, tn, nsplit, s))
            return rc;
        // (only while the planes of the largest split fit)
        if (p->ts_max > nsplit && cap_split_to_planes(p->ts_max, plane) == p->ts_max) {
            a.tsplit = p->d_tsplit;
            a.ts_tile = g.S * (int)kStagedSub;
            a.pos2ph = p->pos2ph;
            nsplit = deep_split = p->ts_max;
        }
    }
    if (deep > 0) {
        if (int rc = layer_split_table(p, nlayers, nsplit, deep, deep_split, s))
            return rc;
        a.unit_tab = p->d_unit_tab;
        a.lsplit = p->d_lsplit;
        a.nunits = p->ut_units;
    }
    const int nunits = deep > 0 ? p->ut_units : nlayers * nsplit;
    a.nsplit = nsplit;
    if (int rc = ensure_part(p, a, deep > 0 ? deep_split : nsplit, s))
        return rc;
    a.ntiles = pb::div_up(wcount, g.S * kStagedSub);
    const int unit_groups = (nunits + 7) / 8;               // (layer, split) units per XCD
    dim3 grid((unsigned)(8 * a.ntiles * unit_groups), a.nrows);
    GatherKernel kern = staged_kernel(g.S, g.dma, a.rows_cap);
    if (int rc = exp_stage_probe_begin(a, g, tn, &kern, s))
        return rc;
    if (int rc = allow_lds(reinterpret_cast<const void *>(kern), g.lds))
        return rc;
    if (int rc = exp_launch_wave(a, nunits, s))
        return rc;
    kern<<<grid, kStagedThreads, g.lds, s>>>(a);
    if (int rc = exp_stage_probe_end(a, s))
        return rc;
    const int32_t *resident = a.res_cap > 0 ? a.ls_resident : nullptr;
    const int64_t per_layer = (int64_t)a.nrows * wcount, n = nlayers * per_layer;
    if (deep > 0) {
        PB_LAUNCH_CHECK();
        dim3 cgrid((unsigned)pb::div_up(per_layer, kBlock), nlayers);
        k_combine_layer_parts<<<cgrid, kBlock, 0, s>>>(a.ext, p->part, p->d_lsplit, per_layer, n,
                                                      resident);
    } else if (a.tsplit) {
        PB_LAUNCH_CHECK();
        if (p->ts_sparse) {
            // the sparse tiles through the global gather (RS = 1: its own 1024-sample tiles;
            // the tiles of the staged kernel end at once there, and the other way round)
            LblArgs ga = a;
            ga.ntiles = pb::div_up(wcount, kTile);
            dim3 ggrid((unsigned)(8 * ga.ntiles * ((nlayers + 7) / 8)), a.nrows);
            k_ext_resample<1, 4><<<ggrid, kBlock, 0, s>>>(ga);
            PB_LAUNCH_CHECK();
        }
        k_combine_tile_parts<<<(unsigned)pb::div_up(n, kBlock), kBlock, 0, s>>>(
            a.ext, p->part, a.tsplit, g.S * (int)kStagedSub, wcount, n, resident, per_layer);
    } else if (nsplit > 1) {
        PB_LAUNCH_CHECK();
        k_combine_parts<<<(unsigned)pb::div_up(n, kBlock), kBlock, 0, s>>>(
            a.ext, p->part, nsplit - 1, n, resident, per_layer);
    }
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int launch_global(LblArgs &a, const Tuning &tn, hipStream_t s)
{
    // record splitting when the launch would not fill the chip
    // (measured at C2: RS=2 beats RS=1 until the launch has ~16k workgroups; a 16-wave
    // workgroup with a 16-way split, selectable with PB_RSPLIT=16, measured slower than
    // RS=4: every wavefront still scans every 64-record round for its share)
    const int64_t tiles1 = pb::div_up(a.wcount, kTile) * (int64_t)a.nlayers * a.nrows;
    const int RS = tn.rsplit ? tn.rsplit : tiles1 >= 16000 ? 1 : tiles1 >= 1500 ? 2 : 4;
    const int tile = RS == 16 ? kWaveSpan : kTile / RS;
    a.ntiles = pb::div_up(a.wcount, tile);
    dim3 grid((unsigned)(8 * a.ntiles * ((a.nlayers + 7) / 8)), a.nrows);
    if (RS == 16)
        k_ext_resample<16, 16><<<grid, 1024, 0, s>>>(a);
    else if (RS == 4)
        k_ext_resample<4, 4><<<grid, kBlock, 0, s>>>(a);
    else if (RS == 2)
        k_ext_resample<2, 4><<<grid, kBlock, 0, s>>>(a);
    else
        k_ext_resample<1, 4><<<grid, kBlock, 0, s>>>(a);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int launch_resident(LblArgs &a, hipStream_t s)
{
    a.ntiles = pb::div_up(a.wcount, kResTile);
    dim3 grid((unsigned)(8 * a.ntiles * ((a.nlayers + 7) / 8)), a.nrows);
    const size_t rlds = ((size_t)a.res_cap + 2) * 8 + (size_t)kResThreads * (16 + 4) +
                        kResWaves * 4 + 64;
    if (int rc = allow_lds(reinterpret_cast<const void *>(k_ext_resident), rlds))
        return rc;
    k_ext_resident<<<grid, kResThreads, rlds, s>>>(a);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace pbx
