// Line-by-line extinction, steps 1 and 2 of the launch sequence (pb_extinction.hip): the state of
// every layer, then the record of every (layer, group) pair with the per-row maximum line strength
// fused in (k_kmax for the plans that keep no records), their launchers, and the counters that read
// the packed records back (pb_lbl_last_work, pb_lbl_last_table_samples).
#include <algorithm>
#include <type_traits>

#include "pb_ext_plan.h"

using namespace pbx;

namespace {

// ---------------------------------------------------------------------------
// 1. per-layer state: one workgroup (64 lanes) per layer, lanes over isotopes
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_layer_state(LblArgs a)
{
    __shared__ unsigned long long s_minwidth;
    __shared__ int s_block;          // largest phase-major profile block any isotope can use
    __shared__ int s_rowmax;         // longest phase row any isotope can select
    // the width grids and the divisors are searched serially by one or a few lanes: one
    // parallel copy into LDS first turns ~40 dependent global loads into LDS reads (the
    // kernel is on the critical path of every spectrum)
    extern __shared__ double s_grid[];                 // lorentz[nlor] | doppler[ndop] | divisors
    double *s_lor = s_grid, *s_dopp = s_grid + a.nlor;
    int *s_div = reinterpret_cast<int *>(s_dopp + a.ndop);
    for (int i = threadIdx.x; i < a.nlor; i += 64)
        s_lor[i] = a.lorentz[i];
    for (int i = threadIdx.x; i < a.ndop; i += 64)
        s_dopp[i] = a.doppler[i];
    for (int i = threadIdx.x; i < a.ndivs; i += 64)
        s_div[i] = a.divisors[i];
    const int layer = blockIdx.x;
    const double temp = a.temp[layer];
    const double fdop = sqrt(2 * pb::kKB * temp / pb::kAMU) * pb::kSqrtLn2 / pb::kLS;
    const double flor = sqrt(2 * pb::kKB * temp / pb::kPi / pb::kAMU) / pb::kLS;
    if (threadIdx.x == 0) {
        s_minwidth = __double_as_longlong(1e5);
        s_block = 0;
        s_rowmax = 0;
    }
    for (int r = threadIdx.x; r < a.nrows; r += 64)
        a.kmax_bits[(int64_t)layer * a.nrows + r] = 0ull;
    __syncthreads();
    const double *dens = a.dens + (int64_t)layer * a.nmol;
    for (int i = threadIdx.x; i < a.niso; i += 64) {
        const int imol = a.isoimol[i];
        double acc = 0.0;
        for (int j = 0; j < a.nmol; j++) {
            double dia = a.molrad[imol] + a.molrad[j];
            acc += dens[j] * dia * dia * sqrt(1 / a.isomass[i] + 1 / a.molmass[j]);
        }
        const double alphal = acc * flor;
        const double alphad = fdop / sqrt(a.isomass[i]);
        const double dw = alphad * a.own0;
        const double vw = 0.5346 * alphal + sqrt(alphal * alphal * 0.2166 + dw * dw);
        atomicMin(&s_minwidth, (unsigned long long)__double_as_longlong(vw));
        const int ilor = pb::nearest_index(s_lor, alphal, 0, a.nlor - 1);
        int hmax = 0;
        for (int d = 0; d < a.ndop; d++)
            hmax = max(hmax, a.psize[ilor * a.ndop + d]);
        // the resident kernel stages whole cells: only the Doppler columns that lines on
        // this grid can select matter (one column of margin on both sides)
        {
            const int dlo = max(0, pb::nearest_index(s_dopp, alphad * a.own0, 0, a.ndop - 1) - 1);
            const int dhi = min(a.ndop - 1,
                                pb::nearest_index(s_dopp, alphad * a.own_last, 0, a.ndop - 1) + 1);
            int used = 0, hlo = INT_MAX, hhi = 0;
            for (int d = dlo; d <= dhi; d++) {
                used = max(used, a.pm_stride[ilor * a.ndop + d]);
                hlo = min(hlo, a.psize[ilor * a.ndop + d]);
                hhi = max(hhi, a.psize[ilor * a.ndop + d]);
            }
            atomicMax(&s_block, used * a.osamp);
            atomicMax(&s_rowmax, used);
            a.li_rowmax[(int64_t)layer * a.niso + i] = used;
            a.li_hlo[(int64_t)layer * a.niso + i] = hlo;
            a.li_hhi[(int64_t)layer * a.niso + i] = hhi;
        }
        const int64_t k = (int64_t)layer * a.niso + i;
        a.li_alphad[k] = alphad;
        a.li_ilor[k] = ilor;
        a.li_hmax[k] = hmax;
        a.li_dens[k] = dens[imol];
        a.li_z[k] = a.isoz[i * a.z_iso_stride + layer * a.z_layer_stride];
        a.li_invz[k] = 1.0 / a.li_z[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double minwidth = __longlong_as_double((long long)s_minwidth);
        int d;
        for (d = 1; d < a.ndivs; d++)
            if (s_div[d] * a.ownstep >= 0.5 * minwidth)
                break;
        const int ofactor = s_div[d - 1];
        a.ls_ofactor[layer] = ofactor;
        a.ls_dwnstep[layer] = a.ownstep * ofactor;
        a.ls_inv_dwnstep[layer] = 1.0 / (a.ownstep * ofactor);
        a.ls_cutsteps[layer] = a.cutoff / (a.ownstep * ofactor);
        a.ls_inv_ofactor[layer] = 1.0 / (double)ofactor;
        a.ls_inv_temp[layer] = 1.0 / temp;
        a.ls_inv_scale[layer] = 1.0 / (double)(int)round(a.wnstep / a.ownstep / ofactor);
        a.ls_dnwn[layer] = 1 + (a.onwn - 1) / ofactor;
        a.ls_scale[layer] = (int)round(a.wnstep / a.ownstep / ofactor);
        a.ls_resident[layer] = a.res_cap > 0 && s_block <= a.res_cap;
        a.ls_block[layer] = s_block;
        // (a resident layer stays the resident kernel's)
        a.ls_wave[layer] = a.wave_cap > 0 && !(a.res_cap > 0 && s_block <= a.res_cap) &&
                           s_rowmax <= a.wave_cap;
    }
}

// ---------------------------------------------------------------------------
// 2. per layer / output row maximum line strength over all in-range lines
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_kmax(LblArgs a, int lines_per_block)
{
    extern __shared__ unsigned long long s_max[];
    const int layer = blockIdx.y;
    if (a.lskip && uniform_load_i32(a.lskip, layer))
        return;
    for (int r = threadIdx.x; r < a.nrows; r += kBlock)
        s_max[r] = 0ull;
    __syncthreads();
    const double temp = a.temp[layer], inv_temp = a.ls_inv_temp[layer];
    const int64_t begin = (int64_t)blockIdx.x * lines_per_block;
    const int64_t end = min(begin + lines_per_block, a.nlines);
    int cur_row = -1;
    double cur_max = 0.0;
    for (int64_t ln = begin + threadIdx.x; ln < end; ln += kBlock) {
        const int i = a.lid[ln];
        int row = a.isoiext[i];
        if (row < 0)
            continue;
        if (a.add)
            row = 0;
        const double v = a.lwn[ln];
        if (v < a.own0 || v > a.own_last)
            continue;
        const int64_t li = (int64_t)layer * a.niso + i;
        const double k = line_strength(a.isoratio[i], a.gf[ln], a.elow[ln], v, temp, inv_temp,
                                       a.li_z[li], a.li_invz[li]);
        if (row != cur_row) {
            if (cur_row >= 0)
                atomicMax(&s_max[cur_row], (unsigned long long)__double_as_longlong(cur_max));
            cur_row = row;
            cur_max = 0.0;
        }
        cur_max = fmax(cur_max, k);
    }
    if (cur_row >= 0)
        atomicMax(&s_max[cur_row], (unsigned long long)__double_as_longlong(cur_max));
    __syncthreads();
    for (int r = threadIdx.x; r < a.nrows; r += kBlock)
        if (s_max[r] != 0ull)
            atomicMax(&a.kmax_bits[(int64_t)layer * a.nrows + r], s_max[r]);
}

// ---------------------------------------------------------------------------
// 2'. Records for the gather kernels: everything about a (layer, group) pair that does
// not depend on the output tile -- co-added strength, table cell and phase row, window on
// the global grid -- is computed ONCE here (coalesced, no workgroup synchronisation) and
// streamed by the gather kernel; the per-row maximum strength (k_kmax) is fused in.
// ---------------------------------------------------------------------------
// kFmt = where the records of the layers walked in phase order go: 0 the six SoA arrays, 1 the
// packed 16-byte records, 2 packed records per (group, chunk of a long row); 3 = every layer
// in position order into 32-byte records (scatter kernel).  Layers of the resident-profile
// kernel are in position order and always use the SoA arrays.  The two orders are two passes
// with their own pointer sets (one body instantiated twice): with both sets and every record
// format live at once the kernel held a third of its scalar state in spilled registers.
// What does not depend on the layer is formed once per thread, before the layer loop: the output
// row and the abundance of the group's isotope, and -- while consecutive layers of the thread
// share their ofactor, a wave-uniform test -- the group's sample of the layer's grid (idwn, one
// FP64 quotient), its sub-sample offset and the cutoff's bounds; the Doppler column is searched
// around the previous layer's.  Figures: profiles/records_diet.md.
template <int kFmt, int kRecLayers>
__global__ __launch_bounds__(kBlock) void k_records(LblArgs a)
{
    extern __shared__ unsigned long long s_max[];                 // [kRecLayers][nrows]
    double *s_dop = reinterpret_cast<double *>(s_max + kRecLayers * a.nrows);   // [ndop]
    const int layer0 = blockIdx.y * kRecLayers;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int r = threadIdx.x; r < kRecLayers * a.nrows; r += kBlock)
        s_max[r] = 0ull;
    for (int d = threadIdx.x; d < a.ndop; d += kBlock)
        s_dop[d] = a.doppler[d];
    // the state of this block's (layer, isotope) pairs, once into LDS: the per-record reads of
    // it were ~12 same-address global loads per layer in a dependent chain
    double *s_alphad = s_dop + a.ndop;                            // [kRecLayers][niso]
    double *s_z = s_alphad + kRecLayers * a.niso;
    double *s_invz = s_z + kRecLayers * a.niso;
    double *s_ratio = s_invz + kRecLayers * a.niso;               // [niso]
    int *s_ilor = reinterpret_cast<int *>(s_ratio + a.niso);      // [kRecLayers][niso]
    int *s_iext = s_ilor + kRecLayers * a.niso;                   // [niso]
    for (int e = threadIdx.x; e < kRecLayers * a.niso; e += kBlock) {
        const int layer = layer0 + e / a.niso;
        if (layer < a.nlayers) {
            const int64_t li = (int64_t)layer * a.niso + e % a.niso;
            s_alphad[e] = a.li_alphad[li];
            s_z[e] = a.li_z[li];
            s_invz[e] = a.li_invz[li];
            s_ilor[e] = a.li_ilor[li];
        }
    }
    for (int e = threadIdx.x; e < a.niso; e += kBlock) {
        s_ratio[e] = a.isoratio[e];
        s_iext[e] = a.isoiext[e];
    }
    int32_t *s_wm = reinterpret_cast<int32_t *>(s_iext + a.niso);  // [wm_n[0] + 1] run offsets
    if (a.wm_off[0] && a.wm_lds)
        for (int e = threadIdx.x; e <= a.wm_n[0]; e += kBlock)
            s_wm[e] = a.wm_off[0][e];
    __syncthreads();
    auto pass = [&](auto posc) {
        constexpr bool kPos = decltype(posc)::value;
        // the group's static data, in the order this pass's gather kernel walks the groups
        int iso = 0, first = 0, count = 0, iown = 0;
        double wavn = 0.0, elow = 0.0, gf = 0.0;
        // A wavenumber shard needs the records of the groups within reach of it only
        // [rec_flo, rec_fhi]; the others still count for the per-row maximum unless the caller
        // all-reduces the maxima of the shards (kmax_local: they are skipped altogether).
        int64_t g = kPos ? t : t + a.grp_lo;                    // (chunked calls: no kPos pass)
        if (a.wm_off[kPos ? 1 : 0]) {
            // run of the window map that holds thread t (the offsets of the phase-order map are
            // in LDS; the position-order map has one run per isotope)
            const int m = kPos ? 1 : 0;
            g = a.ngroups;
            if (t < a.wm_total[m]) {
                const int32_t *off = (kPos || !a.wm_lds) ? a.wm_off[m] : s_wm;
                int lo = 0, hi = a.wm_n[m];                    // last run with off[run] <= t
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (off[mid] <= t)
                        lo = mid;
                    else
                        hi = mid;
                }
                g = (int64_t)a.wm_lo[m][lo] + (t - off[lo]);
            }
        }
        bool have = g < (kPos ? a.ngroups : a.grp_hi), inwin = false;
        if (have) {
            iown = (kPos ? a.giown : a.rk_iown)[g];
            inwin = iown >= a.rec_flo && iown <= a.rec_fhi;
            have = inwin || !a.kmax_local;
        }
        if (have) {
            iso = (kPos ? a.giso : a.rk_iso)[g];
            first = (kPos ? a.gfirst : a.rk_first)[g];
            count = (kPos ? a.gcount : a.rk_count)[g];
            wavn = (kPos ? a.g_lead : a.rk_lwn)[g];                // leader's record
            elow = (kPos ? a.g_lead + a.ngroups : a.rk_elow)[g];
            gf = (kPos ? a.g_lead + 2 * a.ngroups : a.rk_gf)[g];
        }
        // (the lanes that form records are the same in every layer: have, the row and inwin do
        // not depend on it, so what a lane carries from one layer is its own in the next)
        int row0 = -1;
        double ratio = 0.0;
        if (have) {
            row0 = s_iext[iso];
            if (row0 >= 0 && a.add)
                row0 = 0;
            ratio = s_ratio[iso];
        }
        int of_prev = 0, idwn = 0, subw = 0, mincut = 0, maxcut = 0, idop = -1;
        for (int i = 0; i < kRecLayers; i++) {
            const int layer = layer0 + i;
            if (layer >= a.nlayers)
                break;
            const bool pos = kFmt == 3 || (a.res_cap > 0 && uniform_load(a.ls_resident, layer));
            if (pos != kPos)                                          // wave-uniform
                continue;
            const int ofactor = uniform_load(a.ls_ofactor, layer);
            const bool of_new = ofactor != of_prev;                   // wave-uniform
            of_prev = ofactor;
            double k = 0.0, lmax = 0.0;
            int ulo = 0, uhi = 0, q = 0, cell = 0, phi = 0;
            const int row = row0;
            if (have) {
                if (row >= 0) {
                    const int e = i * a.niso + iso;
                    const double temp = uniform_load(a.temp, layer);
                    const double inv_temp = uniform_load(a.ls_inv_temp, layer);
                    const double z = s_z[e], inv_z = s_invz[e];
                    k = line_strength(ratio, gf, elow, wavn, temp, inv_temp, z, inv_z);
                    lmax = k;
                    for (int m = 1; m < count; m++) {
                        const double kp = line_strength(ratio, a.gf[first + m],
                                                        a.elow[first + m], a.lwn[first + m],
                                                        temp, inv_temp, z, inv_z);
                        k += kp;
                        lmax = fmax(lmax, kp);
                    }
                    if (!inwin) {
                        // outside the shard's reach: the strength for the maximum, no record
                        atomicMax(&s_max[i * a.nrows + row],
                                  (unsigned long long)__double_as_longlong(lmax));
                        continue;
                    }
                    const long dnwn = uniform_load(a.ls_dnwn, layer);
                    const double inv_scale = uniform_load(a.ls_inv_scale, layer);
                    // The packed records of the staged gathers keep the window of a group that
                    // leaves the grid UNCLIPPED: their consumers clamp every window to the tile
                    // (hence to the grid) anyway, and the samples below 0 / at or beyond nwave
                    // that the reference's clips `minj = 0`, `maxj = dnwn` remove do not exist
                    // (the upper one only while ceil(dnwn / scale) reaches nwave: checked).
                    // Clipped, every such group had a row window of its own -- one staged row,
                    // one barrier step per RECORD: the first and the last tile of a layer ran
                    // twice as long as the others and ended the launch (904 of 1003 us at C2).
                    constexpr bool kPacked = (kFmt == 1 || kFmt == 2) && !kPos;
                    // (ceil(dnwn / scale) >= nwave in integers: dnwn > (nwave - 1) scale -- scalar
                    // instructions for a wave-uniform value)
                    const int scale = uniform_load(a.ls_scale, layer);
                    const bool hi_free =
                        kPacked && (int64_t)(int)dnwn > (int64_t)(a.nwave - 1) * scale;
                    if (of_new) {
                        // (cutsteps = cutoff / dwnstep follows the factor too)
                        const double cutsteps = uniform_load(a.ls_cutsteps, layer);
                        idwn = trunc_quot_inv(wavn - a.own0, uniform_load(a.ls_dwnstep, layer),
                                              uniform_load(a.ls_inv_dwnstep, layer));
                        subw = iown - idwn * ofactor;
                        mincut = (int)(idwn - cutsteps);
                        maxcut = (int)(idwn + cutsteps);
                    }
                    // (the Doppler column of the thread's previous layer brackets this one's:
                    // alphad moves by a few per cent from layer to layer, a column by more)
                    idop = nearest_index_near(s_dop, s_alphad[e] * wavn, a.ndop, idop);
                    const Window w = window_at<true>(
                        a, idwn, subw, s_ilor[e] * a.ndop + idop, ofactor, dnwn, mincut, maxcut,
                        uniform_load(a.ls_inv_ofactor, layer), !kPacked, !hi_free);
                    // kept samples: minj <= scale*jo < maxj, inside the profile and the grid
                    // (a layer whose grid has the output grid's step -- scale 1, wave-uniform --
                    // needs no quotient)
                    if (scale == 1) {
                        ulo = (int)w.minj;
                        uhi = (int)w.maxj;
                    } else {
                        ulo = -floor_div_inv(-(int)w.minj, inv_scale);
                        uhi = -floor_div_inv(-(int)w.maxj, inv_scale);
                    }
                    q = floor_div_inv(w.half - iown, a.inv_osamp);
                    ulo = max(ulo, -q);
                    uhi = min(uhi, floor_div_inv(iown + w.half, a.inv_osamp) + 1);
                    if (!hi_free)
                        uhi = min(uhi, a.nwave);
                    phi = (w.half - iown) - q * a.osamp;
                    cell = w.cell;
                    if (uhi < ulo)
                        uhi = ulo;
                }
                const int64_t idx = (kFmt == 1 || kFmt == 2) && !kPos
                                        ? (int64_t)layer * a.rec_pitch + (g - a.grp_lo)
                                        : (int64_t)layer * a.ngroups + g;
                if constexpr (kFmt == 3) {
                    Rec32 r;
                    r.k = k;
                    r.off = a.pm_base[cell] + (long long)phi * a.pm_stride[cell] + q;
                    r.ulo = ulo;
                    r.uhi = uhi;
                    r.pad[0] = r.pad[1] = 0;
                    a.rec32[idx] = r;
                } else if constexpr (kFmt == 2 && !kPos) {
                    // long rows (staged in chunks of kChunkRow samples): ONE record per group with
                    // its whole window (14-bit length); the gather clips it to the chunk it
                    // stages.  (Round 2 wrote one record per (group, chunk): 12.8 GB per C3
                    // spectrum, 77 GB per C4 spectrum, written here and streamed back by the gather.)
                    Rec16 r;
                    r.k = k;
                    r.ulo = ulo;
                    r.lc = (uint32_t)(uhi - ulo) | ((uint32_t)cell << kLongLenBits);
                    a.rec16[idx] = r;
                } else if constexpr (kFmt == 1 && !kPos) {
                    Rec16 r;
                    r.k = k;
                    r.ulo = ulo;
                    r.lc = (uint32_t)(uhi - ulo) | ((uint32_t)cell << 12);
                    a.rec16[idx] = r;
                } else {
                    a.rec_k[idx] = k;
                    a.rec_ulo[idx] = ulo;
                    a.rec_uhi[idx] = uhi;
                    a.rec_q[idx] = q;
                    a.rec_cell[idx] = cell;
                    a.rec_phi[idx] = phi;
                }
            }
            if (row >= 0)
                atomicMax(&s_max[i * a.nrows + row],
                          (unsigned long long)__double_as_longlong(lmax));
        }
    };
    if (kFmt != 3)
        pass(std::false_type());
    if (kFmt == 3 || a.res_cap > 0)
        pass(std::true_type());
    __syncthreads();
    for (int r = threadIdx.x; r < kRecLayers * a.nrows; r += kBlock) {
        const int layer = layer0 + r / a.nrows;
        if (layer < a.nlayers && s_max[r] != 0ull)
            atomicMax(&a.kmax_bits[(int64_t)layer * a.nrows + r % a.nrows], s_max[r]);
    }
}

// ---------------------------------------------------------------------------
// Work of the last launch, counted from its packed records (bench.py's roofline.binding):
// out[0] = profile samples multiplied (sum of the live records' windows inside the shard),
// out[1] = lanes the staged kernels issue for them (every 256-sample span a window touches,
// spans aligned to the shard start), out[2] = live records.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_work_stats(LblArgs a, unsigned long long *out)
{
    const int64_t per_layer = (int64_t)a.ngroups;
    const int64_t n = (int64_t)a.nlayers * per_layer;
    const int lbits = a.nch_max > 1 ? kLongLenBits : 12;
    unsigned long long useful = 0, issued = 0, live = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kBlock) {
        const int layer = (int)(i / per_layer);
        const int64_t g = i - (int64_t)layer * a.ngroups;
        const int iext = a.isoiext[a.ph_iso[g]];
        if (iext < 0)
            continue;
        const int row = a.add ? 0 : iext;
        const double kthresh =
            a.ethresh * __longlong_as_double((long long)a.kmax_bits[(int64_t)layer * a.nrows + row]);
        const Rec16 r = a.rec16[i];
        const int64_t ulo = r.ulo, uhi = ulo + (int64_t)(r.lc & ((1u << lbits) - 1u));
        const int64_t lo = max(ulo, a.wbegin) - a.wbegin;
        const int64_t hi = min(uhi, a.wbegin + a.wcount) - a.wbegin;
        if (r.k < kthresh || hi <= lo)
            continue;
        useful += (unsigned long long)(hi - lo);
        if (a.nch_max == 1) {
            issued += (unsigned long long)(((hi - 1) / kStageSpan - lo / kStageSpan + 1) * kStageSpan);
        } else {
            // a long row is visited chunk by chunk: the spans every chunk's part of the window touches
            const int cell = (int)(r.lc >> lbits);
            const int q = floor_div_inv(a.psize[cell] - a.ph_iown[g], a.inv_osamp);
            for (int64_t c0 = 0; c0 < a.rowcap; c0 += kChunkRow) {
                const int64_t clo = max(max(ulo + q, c0) - q, a.wbegin) - a.wbegin;
                const int64_t chi = min(min(uhi + q, c0 + kChunkRow) - q, a.wbegin + a.wcount) - a.wbegin;
                if (chi > clo)
                    issued += (unsigned long long)(((chi - 1) / kStageSpan - clo / kStageSpan + 1) *
                                                   kStageSpan);
            }
        }
        live++;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        useful += __shfl_down(useful, d);
        issued += __shfl_down(issued, d);
        live += __shfl_down(live, d);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], useful);
        atomicAdd(&out[1], issued);
        atomicAdd(&out[2], live);
    }
}

// Distinct Voigt-table samples the live records of the last launch select: per (layer, isotope,
// Doppler column, phase) row the longest window any record takes from it (maxlen, zeroed by the
// caller); the sum of those lengths is what ANY gather must read of the table at least once --
// the operand SURVEY 8(d)'s byte count leaves out.
__global__ __launch_bounds__(kBlock) void k_table_rows(LblArgs a, int32_t *maxlen)
{
    const int64_t n = (int64_t)a.nlayers * a.ngroups;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kBlock) {
        const int layer = (int)(i / a.ngroups);
        const int64_t g = i - (int64_t)layer * a.ngroups;
        const int iso = a.ph_iso[g];
        const int iext = a.isoiext[iso];
        if (iext < 0)
            continue;
        const int row = a.add ? 0 : iext;
        const double kthresh =
            a.ethresh * __longlong_as_double((long long)a.kmax_bits[(int64_t)layer * a.nrows + row]);
        const Rec16 r = a.rec16[i];
        const int len = (int)(r.lc & 0xfffu);
        const int64_t lo = max((int64_t)r.ulo, a.wbegin);
        const int64_t hi = min((int64_t)r.ulo + len, a.wbegin + a.wcount);
        if (r.k < kthresh || hi <= lo)
            continue;
        const int cell = (int)(r.lc >> 12);
        const int idop = cell - a.li_ilor[(int64_t)layer * a.niso + iso] * a.ndop;
        const int d = a.psize[cell] - a.ph_iown[g];
        const int q = floor_div_inv(d, a.inv_osamp);
        const int phi = d - q * a.osamp;
        atomicMax(&maxlen[(((int64_t)layer * a.niso + iso) * a.ndop + idop) * a.osamp + phi], len);
    }
}

__global__ __launch_bounds__(kBlock) void k_sum_i32(const int32_t *v, int64_t n,
                                                    unsigned long long *out)
{
    unsigned long long acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kBlock)
        acc += (unsigned long long)v[i];
    for (int d = 32; d >= 1; d >>= 1)
        acc += __shfl_down(acc, d);
    if ((threadIdx.x & 63) == 0)
        atomicAdd(out, acc);
}

}  // namespace

namespace pbx {

int launch_layer_state(const LblArgs &a, hipStream_t s)
{
    k_layer_state<<<a.nlayers, 64, ((size_t)a.nlor + a.ndop) * 8 + (size_t)a.ndivs * 4, s>>>(a);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int launch_kmax(const LblArgs &a, hipStream_t s)
{
    const int lines_per_block = 4096;
    dim3 grid(pb::div_up(a.nlines, lines_per_block), a.nlayers);
    k_kmax<<<grid, kBlock, (size_t)a.nrows * 8, s>>>(a, lines_per_block);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

// LDS bytes of k_records with `per` layers per thread, before its window-map words
size_t records_lds(const LblArgs &a, int per)
{
    return (size_t)per * a.nrows * 8 + (size_t)a.ndop * 8 +
           (size_t)per * a.niso * (8 + 8 + 8 + 4) + (size_t)a.niso * (8 + 4) + 16;
}

// fmt: 0 SoA records, 1 packed, 2 packed with row chunks, 3 the scatter kernel's.  (The kernels
// lie in the code object in the order they are first named: the packed formats of the usual
// call first, as they always did.)
int launch_records(const LblArgs &a, int fmt, int per, dim3 grid, size_t lds, hipStream_t s)
{
    GatherKernel krec;
    if (per == kRecLayers && (fmt == 1 || fmt == 2))
        krec = fmt == 2 ? k_records<2, kRecLayers> : k_records<1, kRecLayers>;
    else
        krec = per == 1 ? (fmt == 3   ? k_records<3, 1>
                           : fmt == 2 ? k_records<2, 1>
                           : fmt == 1 ? k_records<1, 1>
                                      : k_records<0, 1>)
                        : (fmt == 0 ? k_records<0, kRecLayers> : k_records<3, kRecLayers>);
    krec<<<grid, kBlock, lds, s>>>(a);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace pbx

extern "C" {

int pb_lbl_last_work(pb_lbl *p, int64_t work[3], void *stream)
{
    PB_REQUIRE(p && work, "pb_lbl_last_work: null pointer");
    work[0] = work[1] = work[2] = -1;
    if (!p->last_packed)
        return PB_OK;                 // not counted for this kernel / record format
    hipStream_t s = pb::as_stream(stream);
    unsigned long long *d = nullptr;
    PB_HIP(hipMalloc(&d, 3 * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), s);
    if (e == hipSuccess) {
        k_work_stats<<<1024, kBlock, 0, s>>>(p->last_args, d);
        e = hipGetLastError();
    }
    unsigned long long h[3] = {0, 0, 0};
    if (e == hipSuccess)
        e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    (void)hipFree(d);
    PB_HIP(e);
    for (int i = 0; i < 3; i++)
        work[i] = (int64_t)h[i];
    return PB_OK;
}

int pb_lbl_last_table_samples(pb_lbl *p, int64_t *samples, void *stream)
{
    PB_REQUIRE(p && samples, "pb_lbl_last_table_samples: null pointer");
    *samples = -1;
    const LblArgs &a = p->last_args;
    if (!p->last_packed || a.nch_max != 1)
        return PB_OK;                 // not counted for this kernel / record format
    hipStream_t s = pb::as_stream(stream);
    const int64_t n = (int64_t)a.nlayers * a.niso * a.ndop * a.osamp;
    int32_t *maxlen = nullptr;
    unsigned long long *d = nullptr;
    PB_HIP(hipMalloc(&maxlen, (size_t)n * sizeof(int32_t)));
    hipError_t e = hipMalloc(&d, sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMemsetAsync(maxlen, 0, (size_t)n * sizeof(int32_t), s);
    if (e == hipSuccess)
        e = hipMemsetAsync(d, 0, sizeof(unsigned long long), s);
    unsigned long long h = 0;
    if (e == hipSuccess) {
        k_table_rows<<<1024, kBlock, 0, s>>>(a, maxlen);
        k_sum_i32<<<256, kBlock, 0, s>>>(maxlen, n, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    (void)hipFree(maxlen);
    (void)hipFree(d);
    PB_HIP(e);
    *samples = (int64_t)h;
    return PB_OK;
}

}  // extern "C"
