// Line-by-line extinction for all layers of an atmosphere in one launch sequence.
//
// Restates _extcoeff.extinction (src_c/_extcoeff.c:87-345) as a GATHER:
//
//   reference : per layer, per line group: scatter k*profile[...] over a "dynamic"
//               fine grid (ktmp, up to W*osamp doubles), then keep every
//               (osamp/ofactor)-th sample (resample, utils.h:119-135).
//   here      : the kept samples are computed directly,
//                 ext[jo] = sum_groups k * profile_c[half + osamp*jo - iown],
//               restricted to the reference's window [minj,maxj) of that group
//               (_extcoeff.c:281-299), so ktmp never exists.  The result is the same
//               sum, term for term.
//
// Launch sequence per call (one stream, no host synchronisation; lbl_extinction() at the end of
// this file, which launches what plan_gather() chose):
//   1. k_layer_state : per layer/isotope Lorentz+Doppler widths, width-grid indices,
//                      dynamic-sampling factor (_extcoeff.c:138-200)          [pb_ext_records.hip]
//   2. k_records     : per (layer, group) strength, window and table cell, and with them the per
//                      layer/species maximum line strength (_extcoeff.c:203-226); `resolution`
//                      plans, which keep no records: k_kmax                   [pb_ext_records.hip]
//   3. the gather    : k_ext_resident for the layers with narrow profiles, and for the others
//                      k_ext_staged (+ a k_combine_* pass when a tile's phases were split over
//                      several workgroups) or k_ext_resample (global gather)  [pb_ext_gather.hip];
//                      `resolution` plans: k_ext_linterp / the per-layer dynamic grids of
//                      lbl_resolution_dyn()                                   [pb_ext_resolution.hip]
//      Line lists beyond the record budget repeat 2 and 3 per chunk of the list (run_chunked).
// This file holds the plan handle and its C ABI, the planner (read_tuning, fill_args, plan_gather)
// and the steps that bind the records and order the launches; pb_ext_plan.h declares what the
// files share on the host, pb_ext_args.h what their kernels share.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <new>
#include <vector>

#include "pb_ext_plan.h"

using namespace pbx;

namespace {

// Test aid (PB_POISON_RECORDS=1): new record buffers are filled with LIVE records of an enormous
// strength that select the whole grid from table cell 0, instead of zeros (dead records).  A
// gather kernel that examines a record k_records did not write in this call then shows up as a
// result of ~1e300, not as silence -- tests/test_gpu_extinction.py::test_shards_never_read_unwritten_records.
__global__ __launch_bounds__(kBlock) void k_poison_records(Rec16 *rec16, int64_t n16, Rec32 *rec32,
                                                          int64_t n32, double *rec_k,
                                                          int32_t *rec_i32, int64_t nsoa)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n16; i += stride) {
        Rec16 r;
        r.k = 1e300;
        r.ulo = 0;
        r.lc = 0xfffu;                      // 4095 samples of cell 0
        rec16[i] = r;
    }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n32; i += stride) {
        Rec32 r;
        r.k = 1e300;
        r.off = 0;
        r.ulo = 0;
        r.uhi = INT_MAX;
        r.pad[0] = r.pad[1] = 0;
        rec32[i] = r;
    }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nsoa; i += stride) {
        rec_k[i] = 1e300;
        rec_i32[i] = 0;                     // ulo
        rec_i32[nsoa + i] = INT_MAX;        // uhi
        rec_i32[2 * nsoa + i] = 0;          // q
        rec_i32[3 * nsoa + i] = 0;          // cell
        rec_i32[4 * nsoa + i] = 0;          // phi
    }
}

// ---------------------------------------------------------------------------
// _extcoeff.interp_ec / interp_ec_per_mol (src_c/_extcoeff.c:367-472)
// grid (wavenumber blocks, layers, per_mol ? nmol : 1)
// ---------------------------------------------------------------------------
// kAssign: ext = sum instead of ext += sum (a caller that would zero ext first saves that
// pass and the read: 128 MB of 768 at the C5 shape)
template <bool kAssign>
__global__ __launch_bounds__(kBlock) void k_interp_ec(
    double *ext, const double *etable, const double *ttable, const double *temps,
    const double *density, int nmol, int ntemp, int nlayers, int nwave, int lay1,
    int per_mol)
{
    const int k = lay1 + blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nwave)
        return;
    const double t = temps[k];
    int tlo = pb::nearest_index(ttable, t, 0, ntemp - 1);
    if (t < ttable[tlo] || tlo == ntemp - 1)
        tlo--;
    // A temperature below the table makes the reference read ttable[-1] and etable at a
    // negative offset (_extcoeff.c:394-398; its callers reject such models first,
    // line_sampling.py:426-427).  Here the bracket is clamped -- in-range results are
    // unchanged, an out-of-range layer extrapolates from the first interval -- so a
    // caller that forgot the check gets numbers instead of a GPU fault.
    tlo = max(tlo, 0);
    const int thi = tlo + 1;
    const double span = ttable[thi] - ttable[tlo];
    const double w_lo = (ttable[thi] - t) / span;
    const double w_hi = (t - ttable[tlo]) / span;
    if (per_mol) {
        const int j = blockIdx.z;
        const double d = density[(int64_t)k * nmol + j];
        const double lo = etable[(((int64_t)j * ntemp + tlo) * nlayers + k) * nwave + i];
        const double hi = etable[(((int64_t)j * ntemp + thi) * nlayers + k) * nwave + i];
        double *e = ext + ((int64_t)j * nlayers + k) * nwave + i;
        *e = (kAssign ? 0.0 : *e) + (lo * (w_lo * d) + hi * (w_hi * d));
    } else {
        double acc = kAssign ? 0.0 : ext[(int64_t)k * nwave + i];
        for (int j = 0; j < nmol; j++) {
            const double d = density[(int64_t)k * nmol + j];
            const double lo = etable[(((int64_t)j * ntemp + tlo) * nlayers + k) * nwave + i];
            const double hi = etable[(((int64_t)j * ntemp + thi) * nlayers + k) * nwave + i];
            acc += lo * (w_lo * d) + hi * (w_hi * d);
        }
        ext[(int64_t)k * nwave + i] = acc;
    }
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// LBL plan
// ---------------------------------------------------------------------------
int pb_lbl_create(pb_lbl **out, pb_voigt *voigt, pb_lines *lines, const double *wn_h,
                  int nwave, const int32_t *divisors_h, int ndivs, const double *molrad_h,
                  const double *molmass_h, int nmol, const int32_t *isoimol_h,
                  const double *isomass_h, const double *isoratio_h,
                  const int32_t *isoiext_h, int niso, double cutoff, double ethresh,
                  int resolution, int max_layers)
{
    PB_REQUIRE(out, "pb_lbl_create: null out");
    *out = nullptr;
    PB_REQUIRE(voigt && lines && wn_h && divisors_h && molrad_h && molmass_h && isoimol_h &&
                   isomass_h && isoratio_h && isoiext_h,
               "pb_lbl_create: null pointer");
    PB_REQUIRE(nwave >= 2 && ndivs >= 1 && nmol >= 1 && niso >= 1 && max_layers >= 1,
               "pb_lbl_create: bad sizes");
    PB_REQUIRE(lines->niso == niso, "pb_lbl_create: line list has %d isotopes, got %d",
               lines->niso, niso);
    for (int i = 0; i < niso; i++)
        PB_REQUIRE(isoimol_h[i] >= 0 && isoimol_h[i] < nmol,
                   "pb_lbl_create: isoimol[%d] out of range", i);
    PB_REQUIRE(divisors_h[0] >= 1, "pb_lbl_create: divisors must start at >= 1");
    PB_REQUIRE(resolution || voigt->d_pm || voigt->lazy_parent,
               "pb_lbl_create: this Voigt table keeps the reference layout only (keep_flat = 2); "
               "constant-step plans need the phase-major layout");
    const double wnstep = wn_h[1] - wn_h[0];
    if (!resolution) {
        // the kept samples of every admissible dynamic grid must be osamp apart
        for (int d = 0; d < ndivs; d++) {
            const int scale = (int)round(wnstep / lines->ownstep / divisors_h[d]);
            if ((int64_t)scale * divisors_h[d] != voigt->osamp) {
                pb::set_error("pb_lbl_create: wn step %.9g is not osamp=%d fine steps of "
                              "%.9g for divisor %d",
                              wnstep, voigt->osamp, lines->ownstep, divisors_h[d]);
                return PB_ERR_UNSUPPORTED;
            }
        }
    }
    if (!resolution && lines->onwn >= (1LL << 30)) {
        pb::set_error("pb_lbl_create: fine grid of %lld samples exceeds 2^30", (long long)lines->onwn);
        return PB_ERR_UNSUPPORTED;
    }
    // the gather kernel addresses one Lorentz row of the table with 32-bit offsets
    for (int m = 0; m < voigt->nlor; m++) {
        const size_t k0 = (size_t)m * voigt->ndop, k1 = k0 + voigt->ndop - 1;
        const int64_t span = voigt->pm_base[k1] + (int64_t)voigt->pm_stride[k1] * voigt->osamp -
                             voigt->pm_base[k0] + 4 * (int64_t)kPmPad;
        if (span >= 4294967296LL) {
            pb::set_error("pb_lbl_create: Lorentz row %d of the Voigt table spans %lld "
                          "samples (> 2^32)", m, (long long)span);
            return PB_ERR_UNSUPPORTED;
        }
    }
    pb_lbl *p = new (std::nothrow) pb_lbl();
    if (!p)
        return PB_ERR_NOMEM;
    p->voigt = voigt;
    p->lines = lines;
    p->nwave = nwave;
    p->nmol = nmol;
    p->niso = niso;
    p->ndivs = ndivs;
    p->max_layers = max_layers;
    p->resolution = resolution ? 1 : 0;
#ifdef PB_EXPERIMENTS
    if (const char *e = getenv("PB_RES_DYN_PREDICT"))
        p->dyn_predict = resolution && atoi(e) == 1 ? 1 : 0;
#endif
    p->cutoff = cutoff;
    p->ethresh = ethresh;
    p->wnstep = wnstep;
    p->wn0 = wn_h[0];
    p->isoiext.assign(isoiext_h, isoiext_h + niso);
    if (resolution) {
        p->h_wn.assign(wn_h, wn_h + nwave);
        p->h_divisors.assign(divisors_h, divisors_h + ndivs);
        p->h_molrad.assign(molrad_h, molrad_h + nmol);
        p->h_molmass.assign(molmass_h, molmass_h + nmol);
        p->h_isoimol.assign(isoimol_h, isoimol_h + niso);
        p->h_isoiext0.assign(isoiext_h, isoiext_h + niso);
        p->h_isomass.assign(isomass_h, isomass_h + niso);
        p->h_isoratio.assign(isoratio_h, isoratio_h + niso);
    }
    int rows = 1;
    for (int i = 0; i < niso; i++)
        rows = std::max(rows, isoiext_h[i] + 1);
    p->nrows_sep = rows;
    p->kmax_rows = rows;
    const size_t L = (size_t)max_layers, LI = L * (size_t)niso;
    int rc = PB_OK;
    if (rc == PB_OK) rc = pb::upload(&p->d_wn, wn_h, (size_t)nwave);
    if (rc == PB_OK) rc = pb::upload(&p->d_divisors, divisors_h, (size_t)ndivs);
    if (rc == PB_OK) rc = pb::upload(&p->d_molrad, molrad_h, (size_t)nmol);
    if (rc == PB_OK) rc = pb::upload(&p->d_molmass, molmass_h, (size_t)nmol);
    if (rc == PB_OK) rc = pb::upload(&p->d_isoimol, isoimol_h, (size_t)niso);
    if (rc == PB_OK) rc = pb::upload(&p->d_isomass, isomass_h, (size_t)niso);
    if (rc == PB_OK) rc = pb::upload(&p->d_isoratio, isoratio_h, (size_t)niso);
    if (rc == PB_OK) rc = pb::upload(&p->d_isoiext, isoiext_h, (size_t)niso);
    auto alloc = [&](void **ptr, size_t bytes) {
        if (rc == PB_OK && hipMalloc(ptr, bytes) != hipSuccess) {
            pb::set_error("pb_lbl_create: workspace allocation failed");
            rc = PB_ERR_NOMEM;
        }
    };
    alloc((void **)&p->ls_ofactor, L * 4);
    alloc((void **)&p->ls_scale, L * 4);
    alloc((void **)&p->ls_dnwn, L * 8);
    alloc((void **)&p->ls_dwnstep, L * 8);
    alloc((void **)&p->ls_quot, 5 * L * 8);
    alloc((void **)&p->li_invz, LI * 8);
    alloc((void **)&p->li_alphad, LI * 8);
    alloc((void **)&p->li_dens, LI * 8);
    alloc((void **)&p->li_z, LI * 8);
    alloc((void **)&p->li_ilor, LI * 4);
    alloc((void **)&p->li_hmax, LI * 4);
    alloc((void **)&p->li_rowmax, LI * 4);
    alloc((void **)&p->li_hlo, LI * 4);
    alloc((void **)&p->li_hhi, LI * 4);
    alloc((void **)&p->kmax_bits, L * (size_t)rows * 8);
    alloc((void **)&p->ls_resident, L * 4);
    alloc((void **)&p->ls_block, L * 4);
    alloc((void **)&p->ls_wave, L * 4);
    // the whole buffer is what a multi-GPU run all-reduces (pb_lbl_kmax_buffer): slots beyond the
    // rows of a call must not hold whatever the allocation did
    if (rc == PB_OK && hipMemset(p->kmax_bits, 0, L * (size_t)rows * 8) != hipSuccess)
        rc = PB_ERR_HIP;
    if (rc == PB_OK && !resolution) {
        // groups re-sorted by (isotope, iown mod osamp, iown): all lines that read the same
        // phase row of a profile become neighbours (k_ext_staged)
        const int osamp = voigt->osamp;
        const size_t ng = lines->h_giown.size();
        // counting sort by phase inside every isotope (stable: positions stay ascending); a
        // comparison sort with a modulo in its comparator took 1.3 s at 1e7 lines
        std::vector<int32_t> order(ng);
        std::vector<int64_t> start((size_t)niso * (osamp + 1) + 1, 0);
        for (int i = 0; i < niso; i++) {
            const int64_t s0 = lines->iso_gstart[i], s1 = lines->iso_gstart[i + 1];
            std::vector<int64_t> cnt((size_t)osamp + 1, 0);
            for (int64_t k = s0; k < s1; k++)
                cnt[(size_t)(lines->h_giown[k] % osamp) + 1]++;
            int64_t run = s0;
            for (int ph = 0; ph <= osamp; ph++) {
                run += cnt[ph];
                start[(size_t)i * (osamp + 1) + ph] = run;
            }
            // start[ph] = first slot AFTER phase ph-1 ... re-derive the first slot of each phase
            std::vector<int64_t> slot((size_t)osamp, 0);
            int64_t at = s0;
            for (int ph = 0; ph < osamp; ph++) {
                slot[ph] = at;
                at += cnt[(size_t)ph + 1];
            }
            for (int64_t k = s0; k < s1; k++)
                order[(size_t)slot[(size_t)(lines->h_giown[k] % osamp)]++] = (int32_t)k;
        }
        start[(size_t)niso * (osamp + 1)] = (int64_t)ng;
        std::vector<int32_t> f(ng), c(ng), w(ng);
        for (size_t k = 0; k < ng; k++) {
            f[k] = lines->h_gfirst[order[k]];
            c[k] = lines->h_gcount[order[k]];
            w[k] = lines->h_giown[order[k]];
        }
        {
            std::vector<int32_t> inv(ng);                 // position-sorted group -> phase-sorted slot
            for (size_t k = 0; k < ng; k++)
                inv[(size_t)order[k]] = (int32_t)k;
            if (rc == PB_OK) rc = pb::upload(&p->pos2ph, inv.data(), ng);
        }
        if (rc == PB_OK) rc = pb::upload(&p->ph_first, f.data(), ng);
        if (rc == PB_OK) rc = pb::upload(&p->ph_count, c.data(), ng);
        if (rc == PB_OK) rc = pb::upload(&p->ph_iown, w.data(), ng);
        if (rc == PB_OK) rc = pb::upload(&p->ph_start, start.data(), start.size());
        p->h_ph_iown = w;
        p->h_ph_start = start;
        {
            // position index of every (isotope, phase) run, one entry per kBinSamples samples
            const int nbins = (int)pb::div_up((int64_t)nwave, (int64_t)kBinSamples) + 1;
            const int64_t binw = (int64_t)kBinSamples * osamp;
            std::vector<int32_t> bins((size_t)niso * osamp * ((size_t)nbins + 1));
            for (int i = 0; i < niso; i++)
                for (int ph = 0; ph < osamp; ph++) {
                    int64_t k = start[(size_t)i * (osamp + 1) + ph];
                    const int64_t kend = start[(size_t)i * (osamp + 1) + ph + 1];
                    int32_t *row = bins.data() + ((size_t)i * osamp + ph) * ((size_t)nbins + 1);
                    for (int b = 0; b < nbins; b++) {
                        while (k < kend && (int64_t)w[(size_t)k] < b * binw)
                            k++;
                        row[b] = (int32_t)k;
                    }
                    row[nbins] = (int32_t)kend;
                }
            p->ph_nbins = nbins;
            if (rc == PB_OK) rc = pb::upload(&p->ph_bin, bins.data(), bins.size());
        }
        {
            std::vector<int32_t> iso_of(ng);
            for (int i = 0; i < niso; i++)
                for (int64_t k = lines->iso_gstart[i]; k < lines->iso_gstart[i + 1]; k++)
                    iso_of[(size_t)k] = i;
            if (rc == PB_OK) rc = pb::upload(&p->ph_iso, iso_of.data(), ng);
        }
        {
            // leader line of every group in both walk orders (coalesced reads in k_records)
            const std::vector<double> &lwn_all = lines->h_lwn, &elow_all = lines->h_elow,
                                      &gf_all = lines->h_gf;
            std::vector<double> lead(3 * ng), glead(3 * ng);
            for (size_t k = 0; k < ng; k++) {
                const int32_t lf = f[k], gf_ = lines->h_gfirst[k];
                lead[k] = lwn_all[lf];
                lead[ng + k] = elow_all[lf];
                lead[2 * ng + k] = gf_all[lf];
                glead[k] = lwn_all[gf_];
                glead[ng + k] = elow_all[gf_];
                glead[2 * ng + k] = gf_all[gf_];
            }
            if (rc == PB_OK) rc = pb::upload(&p->ph_lead, lead.data(), lead.size());
            if (rc == PB_OK) rc = pb::upload(&p->g_lead, glead.data(), glead.size());
        }
        // per (layer, group) records of k_records: allocated on first use
        int cap = 0, smallest = INT_MAX;
        for (int32_t st : voigt->pm_stride) {
            cap = std::max(cap, st);
            smallest = std::min(smallest, st);
        }
        p->rowcap = cap;
        // resident-profile kernel: 64 KiB of LDS for one cell's phase-major block
        if (ng > 0 && (int64_t)smallest * osamp <= kResCapDefault)
            p->res_cap = kResCapDefault;
        if (const char *e = getenv("PB_RESIDENT_CAP"))
            p->res_cap = std::max(0, std::min(atoi(e), 19000));
        if (p->res_cap > 0) {
            // first position-sorted group of every isotope at or after each output sample
            std::vector<int32_t> gs((size_t)niso * ((size_t)nwave + 1));
            for (int i = 0; i < niso; i++) {
                int64_t g = lines->iso_gstart[i];
                const int64_t gend = lines->iso_gstart[i + 1];
                for (int64_t w = 0; w <= nwave; w++) {
                    while (g < gend && (int64_t)lines->h_giown[(size_t)g] < w * osamp)
                        g++;
                    gs[(size_t)i * ((size_t)nwave + 1) + (size_t)w] = (int32_t)g;
                }
            }
            if (rc == PB_OK) rc = pb::upload(&p->gs_start, gs.data(), gs.size());
        }
    }
    {
        const char *e = getenv("PB_GATHER");
        if (e && !strcmp(e, "global"))
            p->gather_mode = 1;
        else if (e && !strcmp(e, "staged"))
            p->gather_mode = 2;
        else if (e && !strcmp(e, "resident"))
            p->gather_mode = 3;
#ifdef PB_EXPERIMENTS
        else if (e && !strcmp(e, "scatter"))
            p->gather_mode = 4;
        else if (e && !strcmp(e, "rounds"))
            p->gather_mode = 5;
#endif
        const char *t = getenv("PB_STAGE_THRESHOLD");
        if (t)
            p->stage_threshold = atof(t);
    }
    if (rc != PB_OK) {
        pb_lbl_destroy(p);
        return rc;
    }
    *out = p;
    return PB_OK;
}

int pb_lbl_set_isoiext(pb_lbl *p, const int32_t *isoiext_h)
{
    PB_REQUIRE(p && isoiext_h, "pb_lbl_set_isoiext: null pointer");
    for (int i = 0; i < p->niso; i++)
        PB_REQUIRE(isoiext_h[i] < p->kmax_rows,
                   "pb_lbl_set_isoiext: row %d exceeds the %d rows of the plan",
                   isoiext_h[i], p->kmax_rows);
    p->isoiext.assign(isoiext_h, isoiext_h + p->niso);
    PB_HIP(hipMemcpy(p->d_isoiext, isoiext_h, (size_t)p->niso * 4, hipMemcpyHostToDevice));
    return PB_OK;
}

int pb_lbl_set_gather_mode(pb_lbl *p, int mode)
{
    PB_REQUIRE(p && mode >= 0 && mode <= 7, "pb_lbl_set_gather_mode: mode must be 0..7");
#ifndef PB_EXPERIMENTS
    PB_REQUIRE(mode != 4 && mode != 5 && mode != 7,
               "pb_lbl_set_gather_mode: mode %d (scatter / rounds / wave) is a measured dead end "
               "kept out of libpbhip.so: `make -C pyratbay_amd/csrc EXPERIMENTS=1` builds "
               "libpbhip_exp.so with it", mode);
#endif
    PB_REQUIRE(mode != 6 || p->resolution,
               "pb_lbl_set_gather_mode: mode 6 (per-layer dynamic grids) is for `resolution` plans");
    p->gather_mode = mode;
    return PB_OK;
}

int pb_lbl_set_record_budget(pb_lbl *p, int64_t bytes)
{
    PB_REQUIRE(p && bytes >= (int64_t)sizeof(Rec16), "pb_lbl_set_record_budget: bad budget");
    p->record_budget = (size_t)bytes;
    return PB_OK;
}

int pb_lbl_last_chunks(const pb_lbl *p, int *chunks)
{
    PB_REQUIRE(p && chunks, "pb_lbl_last_chunks: null pointer");
    *chunks = p->last_chunks;
    return PB_OK;
}

int pb_lbl_set_concurrency(pb_lbl *p, int n)
{
    PB_REQUIRE(p && n >= 1, "pb_lbl_set_concurrency: n must be >= 1");
    p->concurrency = n;
    return PB_OK;
}

int pb_lbl_last_gather_mode(const pb_lbl *p, int *mode)
{
    PB_REQUIRE(p && mode, "pb_lbl_last_gather_mode: null pointer");
    *mode = p->last_gather;
    return PB_OK;
}

int pb_lbl_set_ethresh(pb_lbl *p, double ethresh)
{
    PB_REQUIRE(p, "pb_lbl_set_ethresh: null handle");
    p->ethresh = ethresh;
    return PB_OK;
}

}  // extern "C"

namespace pbx {

// ---------------------------------------------------------------------------
// one extinction call: environment, arguments, plan, then the steps in launch order
// ---------------------------------------------------------------------------
static Tuning read_tuning()
{
    Tuning t;
    auto is_zero = [](const char *name) {
        const char *e = getenv(name);
        return e && atoi(e) == 0;
    };
    if (const char *e = getenv("PB_EXPERIMENT"))
        t.experiment = atoi(e);
    t.dma = !is_zero("PB_STAGE_DMA");
    t.no_long_rows = getenv("PB_NO_LONG_ROWS") != nullptr;
    if (const char *e = getenv("PB_STAGE_S"))
        t.stage_s = atoi(e) >= 4 ? 4 : atoi(e) >= 2 ? 2 : 1;
    if (const char *e = getenv("PB_STAGE_SPLIT"))
        t.stage_split = std::max(1, std::min(8, atoi(e)));
    if (const char *e = getenv("PB_STAGE_ROWS"))
        t.stage_rows = std::max(1, std::min(kStageRowsMax, atoi(e)));
    if (const char *e = getenv("PB_POISON_RECORDS"))
        t.poison = atoi(e) != 0;
    if (const char *e = getenv("PB_RECORD_BUDGET")) {
        t.budget_set = true;
        t.budget = (size_t)atoll(e);
    }
    t.rec_soa = getenv("PB_REC_SOA") != nullptr;
    t.res_dyn_off = is_zero("PB_RES_DYN");
    if (const char *e = getenv("PB_REC_LAYERS"))
        t.rec_layers_1 = atoi(e) == 1;
    t.no_window_map = getenv("PB_NO_WINDOW_MAP") != nullptr;
    if (const char *e = getenv("PB_WM_LDS_CAP"))
        t.wm_lds_cap = (size_t)atol(e);
    if (const char *e = getenv("PB_STAGE_DEEP")) {
        t.deep_set = true;
        t.deep_frac = atof(e);
        if (const char *c = strchr(e, ','))
            t.deep_factor = std::max(1, atoi(c + 1));
    }
    t.tile_split_off = is_zero("PB_TILE_SPLIT");
    if (const char *e = getenv("PB_TILE_MIN"))
        t.tile_min = atoi(e);
    t.tile_debug = getenv("PB_TILE_DEBUG") != nullptr;
    t.tile_global_off = is_zero("PB_TILE_GLOBAL");
    if (const char *e = getenv("PB_RSPLIT")) {
        const int v = atoi(e);
        t.rsplit = v >= 16 ? 16 : v >= 4 ? 4 : v >= 2 ? 2 : 1;
    }
    if (const char *e = getenv("PB_RES_DYN_STREAMS"))
        t.dyn_streams = std::max(1, std::min(8, atoi(e)));
    if (const char *e = getenv("PB_RES_DYN_BIG"))
        t.dyn_big = std::max(1, std::min(7, atoi(e)));
    if (kExp) {
        if (const char *e = getenv("PB_WAVE"))
            t.wave = atoi(e) != 0 ? 1 : 0;
        if (const char *e = getenv("PB_SCATTER_T"))
            t.scatter_t = atoi(e) >= 2048 ? 2048 : atoi(e) >= 1024 ? 1024 : 512;
        if (const char *e = getenv("PB_ROUNDS_GEOM"))
            t.rounds_geom = std::max(0, std::min(7, atoi(e)));
        if (const char *e = getenv("PB_STAGE_PROBE"))
            t.stage_probe = atoi(e);
    }
    return t;
}

// The largest distance (fine samples) from which a group can reach an output sample, over all
// layers: the widest profile of the table, or the cutoff where that is shorter.
int64_t group_reach(const pb_voigt *v, double cutoff, double ownstep)
{
    int64_t hmax_all = 0;
    for (int32_t h : v->psize)
        hmax_all = std::max<int64_t>(hmax_all, h);
    int64_t reach = hmax_all;
    if (cutoff > 0.0)
        reach = std::min(reach, (int64_t)(cutoff / ownstep) + 2 * (int64_t)v->osamp + 2);
    return reach;
}

// groups (any isotope) at fine positions [flo, fhi]: host copy of the position-sorted list
int64_t groups_in_reach(const pb_lines *l, int niso, int64_t flo, int64_t fhi)
{
    int64_t n = 0;
    for (int i = 0; i < niso; i++) {
        const int32_t *b = l->h_giown.data() + l->iso_gstart[(size_t)i];
        const int32_t *e = l->h_giown.data() + l->iso_gstart[(size_t)i + 1];
        n += std::upper_bound(b, e, (int32_t)std::min<int64_t>(fhi, INT_MAX)) -
             std::lower_bound(b, e, (int32_t)std::max<int64_t>(flo, INT_MIN));
    }
    return n;
}

// the part of LblArgs that follows from the plan and the call alone (everything else is zero)
static LblArgs fill_args(const pb_lbl *p, const Call &c)
{
    const pb_voigt *v = p->voigt;
    const pb_lines *l = p->lines;
    LblArgs a;
    memset(&a, 0, sizeof(a));
    a.pm = v->d_pm;
    a.flat = v->d_flat;
    a.pm_base = v->d_pm_base;
    a.pm_stride = v->d_pm_stride;
    a.psize = v->d_psize;
    a.pindex = v->d_pindex;
    a.doppler = v->d_doppler;
    a.lorentz = v->d_lorentz;
    a.ndop = v->ndop;
    a.nlor = v->nlor;
    a.osamp = v->osamp;
    a.lwn = l->d_lwn;
    a.elow = l->d_elow;
    a.gf = l->d_gf;
    a.lid = l->d_lid;
    a.gfirst = l->d_gfirst;
    a.gcount = l->d_gcount;
    a.giown = l->d_giown;
    a.iso_gstart = l->d_iso_gstart;
    a.nlines = l->nlines;
    a.ph_first = p->ph_first;
    a.ph_count = p->ph_count;
    a.ph_iown = p->ph_iown;
    a.ph_start = p->ph_start;
    a.rowcap = p->rowcap;
    a.ph_iso = p->ph_iso;
    a.ph_bin = p->ph_bin;
    a.ph_nbins = p->ph_nbins;
    a.g_lead = p->g_lead;
    a.ls_resident = p->ls_resident;
    a.ls_block = p->ls_block;
    a.ls_wave = p->ls_wave;
    a.gs_start = p->gs_start;
    a.giso = l->d_giso;
    a.ngroups = l->ngroups;
    a.inv_osamp = 1.0 / (double)v->osamp;
    a.molrad = p->d_molrad;
    a.molmass = p->d_molmass;
    a.isoimol = p->d_isoimol;
    a.isoiext = p->d_isoiext;
    a.isomass = p->d_isomass;
    a.isoratio = p->d_isoratio;
    a.divisors = p->d_divisors;
    a.nmol = p->nmol;
    a.niso = p->niso;
    a.ndivs = p->ndivs;
    a.temp = c.temp;
    a.dens = c.dens;
    a.isoz = c.isoz;
    a.z_iso_stride = c.zs0;
    a.z_layer_stride = c.zs1;
    a.ls_ofactor = p->ls_ofactor;
    a.ls_scale = p->ls_scale;
    a.ls_dnwn = p->ls_dnwn;
    a.ls_dwnstep = p->ls_dwnstep;
    a.ls_cutsteps = p->ls_quot;
    a.ls_inv_ofactor = p->ls_quot + p->max_layers;
    a.ls_inv_scale = p->ls_quot + 2 * (size_t)p->max_layers;
    a.ls_inv_temp = p->ls_quot + 3 * (size_t)p->max_layers;
    a.ls_inv_dwnstep = p->ls_quot + 4 * (size_t)p->max_layers;
    a.li_invz = p->li_invz;
    a.li_alphad = p->li_alphad;
    a.li_dens = p->li_dens;
    a.li_z = p->li_z;
    a.li_ilor = p->li_ilor;
    a.li_hmax = p->li_hmax;
    a.li_rowmax = p->li_rowmax;
    a.li_hlo = p->li_hlo;
    a.li_hhi = p->li_hhi;
    a.kmax_bits = p->kmax_bits;
    a.wn = p->d_wn;
    a.own0 = l->own0;
    a.own_last = l->own_last;
    a.ownstep = l->ownstep;
    a.wnstep = p->wnstep;
    a.wn0 = p->wn0;
    a.onwn = l->onwn;
    a.cutoff = p->cutoff;
    a.ethresh = p->ethresh;
    a.add = c.add ? 1 : 0;
    a.nrows = c.add ? 1 : p->nrows_sep;
    a.nlayers = c.nlayers;
    a.nwave = p->nwave;
    a.wbegin = c.wbegin;
    a.wcount = c.wcount;
    a.ext = c.ext;
    // records are needed for the groups within reach of the shard only.  The window must hold
    // every group ANY gather kernel may examine: the staged / global / round kernels bracket
    // their candidates by fine position (within min(hmax, cutoff) + osamp + ofactor of a tile),
    // the resident and scatter kernels through the per-sample index gs_start, which examines
    // up to two more output samples' worth of groups on either side -- hence 6 (not 2) x osamp
    // of margin.  A group examined but never written would be whatever the allocation held
    // (round 2: garbage records of a long-lived process sent the resident kernel out of
    // bounds; found by tools/fuzz_pipeline.py); the buffers are also zeroed when allocated, so
    // a record never written is a dead record.
    const int64_t reach = group_reach(v, a.cutoff, a.ownstep) + 6 * (int64_t)v->osamp;
    const bool whole = c.wbegin == 0 && c.wcount == p->nwave;
    a.rec_flo = whole ? INT64_MIN : c.wbegin * (int64_t)v->osamp - reach;
    a.rec_fhi = whole ? INT64_MAX : (c.wbegin + c.wcount - 1) * (int64_t)v->osamp + reach;
    // every group in one piece, one workgroup per tile: the chunked walk and the phase splits
    // narrow these
    a.grp_hi = l->ngroups;
    a.rec_pitch = l->ngroups;
    a.key_hi = a.niso * v->osamp;
    a.nsplit = 1;
    return a;
}

// Grow *ptr to `need` bytes (*have = its size so far); what it held is lost.  sync_first: an
// earlier call on the stream may still read the old block.  Running out of memory is
// PB_ERR_NOMEM "cannot allocate <need> B of <what>"; without `what`, the runtime's own error.
int ensure_bytes(void **ptr, size_t *have, size_t need, hipStream_t s, bool sync_first,
                 const char *what)
{
    if (need <= *have)
        return PB_OK;
    if (*ptr) {
        if (sync_first)
            PB_HIP(hipStreamSynchronize(s));
        (void)hipFree(*ptr);
        *ptr = nullptr;
        *have = 0;
    }
    if (!what)
        PB_HIP(hipMalloc(ptr, need));
    else if (hipMalloc(ptr, need) != hipSuccess) {
        pb::set_error("pb_lbl_extinction: cannot allocate %zu B of %s", need, what);
        return PB_ERR_NOMEM;
    }
    *have = need;
    return PB_OK;
}

// bytes of one plane of partial sums, and the largest split <= n (>= least) whose planes beside
// ext stay below 1 GiB
int64_t plane_bytes(const LblArgs &a)
{
    return (int64_t)a.nlayers * a.nrows * a.wcount * 8;
}

int cap_split_to_planes(int n, int64_t plane, int least)
{
    while (n > least && (n - 1) * plane > ((int64_t)1 << 30))
        n--;
    return n;
}

// partial sums of a launch split into `nplanes` pieces (the first piece writes ext itself)
int ensure_part(pb_lbl *p, LblArgs &a, int nplanes, hipStream_t s)
{
    if (nplanes <= 1)
        return PB_OK;
    const size_t need = (size_t)(nplanes - 1) * a.nlayers * a.nrows * a.wcount * 8;
    if (int rc = ensure_bytes((void **)&p->part, &p->part_bytes, need, s, false, "partial sums"))
        return rc;
    a.part = p->part;
    return PB_OK;
}

// Makes no HIP call and does not write to *p.  The two pieces of state the choice touches are
// applied by the caller (resident_probe): whether the stream is being captured, and the plan's
// probe counter and pending decision (res_calls, res_on_pending, res_look_pending).
static GatherPlan plan_gather(const pb_lbl *p, const LblArgs &a, const Tuning &tn, int phase)
{
    const pb_voigt *v = p->voigt;
    const pb_lines *l = p->lines;
    const int nlayers = a.nlayers;
    const int64_t wcount = a.wcount;
    GatherPlan g;
    // Kernel choice (constant-step grids): the LDS-staged kernel when several groups share
    // a (tile, phase) row, else the global gather.  Every kernel adds the terms of a sample in
    // one fixed order, so a call is bitwise reproducible and shards of ONE configuration
    // concatenate exactly; the choice of kernel and the phase split below do depend on the size
    // of the call (shard width, layers), and a different choice changes the association of the
    // per-sample sums: results of different configurations agree to ~1e-13, not bit for bit.
    // rows longer than kStageRowMax samples are staged in chunks: (phase, chunk) pairs act as
    // phases; k_records writes one packed record per group, clipped to the chunk by the gather
    const int nch_max = std::max(1, (int)pb::div_up((int64_t)a.rowcap, (int64_t)kChunkRow));
    g.rowlds = (std::min(a.rowcap, kStageRowMax) + 1) & ~1;     // even: 16-byte aligned buffers
    const size_t lds_fixed = (size_t)kStagedThreads * (16 + 8 + 4) + kStagedWaves * 12 +
                             (size_t)a.ndop * 16 +
                             (size_t)(2 * v->osamp * nch_max + 1) * 4 + 64;
    g.dma = tn.dma;
    g.lds = (2 * ((size_t)g.rowlds + kStagePad) + kStagePad) * 8 + lds_fixed;
    const double per_phase = (double)l->ngroups / std::max(1, p->nwave) * 2048.0 / v->osamp;
    g.per_phase = per_phase;
    // table cell and window length share 32 bits of a packed record: 20 + 12, for long rows
    // 18 + kLongLenBits (windows of up to 16 383 samples)
    const bool packable = v->nlor * v->ndop < (nch_max > 1 ? (1 << (32 - kLongLenBits)) : (1 << 20)) &&
                          a.rowcap < (1 << kLongLenBits);
    g.packable = packable;
    // sized for the layers of this call (a layer shard of a multi-GPU run holds few of them)
    const size_t rec16_bytes = (size_t)nlayers * (size_t)l->ngroups * sizeof(Rec16);
    const bool can_stage = !p->resolution && g.lds <= 160 * 1024 && l->ngroups > 0 &&
                           (nch_max == 1 || (nch_max <= 16 && packable && !tn.no_long_rows));
    // the staged kernel needs enough workgroups to hide its per-segment latency; launches that
    // stay below 750 even when split eight ways go to the global gather with record splitting.
    // Tiling of the staged kernel: S = 2 sub-tiles of 2048 samples per workgroup (1 measured
    // slower at every launch size once the splits are spread over the XCDs; 4 spills: 32
    // accumulators at the 64-register budget) and nsplit workgroups per tile, each with its
    // share of the phases.  A launch ends when its slowest workgroup does, so small launches
    // and launches of long-running workgroups are split further:
    //  * light tiles (C2: ~8 records per phase row): aim for ~2000 workgroups.  Layer shards
    //    of C2 (a sweep of round 2): 40 layers       0.70 ms unsplit / 0.65 in two; 20 layers
    //    0.40 in two / 0.37 in four; 10 layers 0.23 in four or eight; all 80 layers 1.19
    //    unsplit / 1.20 in two.
    //  * heavy tiles (>= 64 groups per phase row and 2048 samples: 1e6 lines on 1e5 samples;
    //    a workgroup then runs for milliseconds): aim for ~8000.  1e6 lines, 80 layers:
    //    8.13 ms unsplit, 7.33 in four; a 10-layer shard 2.03 -> 1.13 in eight.
    // The partial sums stay below 1 GB.
    const int64_t sub = kStagedSub;
    const int64_t blocks2 = pb::div_up(wcount, 2 * sub) * (int64_t)nlayers;
    // With other spectra in flight on other streams (pb_lbl_set_concurrency: the walkers of a
    // retrieval, the pipelined shards of a multi-GPU rank) a launch need not fill the chip by
    // itself: one round of workgroups (~1000) amortises the per-workgroup candidate search
    // better.  A 1/8 wavenumber shard of C2, two-phase, per spectrum: one at a time 0.269-0.277
    // ms whatever the split; two in flight 0.211 (3 workgroups per 4096-sample tile = 960, one round; 4 per tile: 0.232) against
    // 0.240 (7 per 2048-sample tile, the one-at-a-time rule); three in flight 0.190 against 0.236.
    const bool shared_chip = p->concurrency > 1 && per_phase < 64.0;
    g.shared_chip = shared_chip;
    int S = 2;
    int nsplit = (int)std::min<int64_t>(
        8, pb::div_up((int64_t)(per_phase >= 64.0 ? 8000 : 2000), std::max<int64_t>(1, blocks2)));
    if (shared_chip) {
        // the ~2000 workgroups of the rule above, counted over ALL the spectra in flight.  (Until
        // the rank loop stopped being host-bound -- second session of round 3 -- one round of 1024
        // per launch measured best; with the host out of the way, a 1/8 shard of C2 with three in
        // flight: 1 / 2 / 3 / 4 pieces per tile 0.211 / 0.163 / 0.179 / 0.181 ms per spectrum, a
        // 1/4 shard 0.276 / 0.279 / 0.291, a 1/2 shard 0.467 / 0.502.)
        const int64_t inflight = blocks2 * std::max(1, p->concurrency);
        nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(8, (2000 + inflight / 2) / std::max<int64_t>(1, inflight)));
    }
    nsplit = cap_split_to_planes(nsplit, plane_bytes(a));
    {
        // tile quantisation of a narrow shard: 12 500 samples are 3.05 tiles of 4096 (31 % of
        // the workgroups' rows staged for nothing) but 6.1 of 2048 (15 %); one span per
        // workgroup when that saves more than 12 % (N = 8 shards of C2: 0.305 -> 0.297 ms, of the
        // 1e6-line list 1.47 -> 1.28 ms; N = 4: the two-span tile stays faster).  The sums do not
        // depend on S (tests/test_gpu_extinction.py::test_staged_variants_agree).
        const double w2 = (double)pb::div_up(wcount, 2 * sub) * 2 * sub / (double)wcount;
        const double w1 = (double)pb::div_up(wcount, sub) * sub / (double)wcount;
        if (w2 - w1 > 0.12 && !shared_chip)
            S = 1;
    }
    if (tn.stage_s)
        S = tn.stage_s;
    if (tn.stage_split)
        nsplit = tn.stage_split;
    g.S = S;
    g.nsplit = nsplit;
    // (with other spectra in flight the launches of all of them count towards filling the chip)
    const bool enough_blocks = pb::div_up(wcount, S * sub) * (int64_t)nlayers * nsplit *
                                   (shared_chip ? p->concurrency : 1) >= 750;
    // round-staged kernel (pb_rounds.hip): rows of one piece (<= 1024 samples), packed records
    const bool rounds = kExp && can_stage && nch_max == 1 && packable && p->gather_mode == 5;
    const bool staged = can_stage && (p->gather_mode == 2 || p->gather_mode == 7 || rounds ||
                                      (p->gather_mode == 0 && enough_blocks &&
                                       per_phase >= p->stage_threshold));
    const bool use_records = !p->resolution && l->ngroups > 0;
    // layers with narrow profiles go to the resident-profile kernel (decided per layer on
    // the device, from the layer alone); the kernel chosen above computes the others
    const bool scatter = kExp && use_records && p->gs_start && p->gather_mode == 4;
    g.rounds = rounds;
    g.staged = staged;
    g.use_records = use_records;
    g.scatter = scatter;
    g.resident = use_records && !scatter && p->res_cap > 0 && p->gs_start &&
                 (p->gather_mode == 0 || p->gather_mode == 3);
    g.res_auto = g.resident && p->gather_mode == 0;
    // (the LDS of the staged kernel above was sized for the row chunks even so)
    g.nch_max = !staged || scatter ? 1 : nch_max;
    // Out-of-core line lists (the reference walks any number of lines one after the other,
    // _extcoeff.c:203-309): when the packed records of all groups exceed the record budget, the
    // phase-sorted group list is cut into chunks of consecutive (isotope, phase) keys that fit.
    const size_t budget = tn.budget_set ? tn.budget : p->record_budget;
    g.rec16_need = rec16_bytes;
    if (staged && !scatter && rec16_bytes > budget) {
        if (!packable || rounds || phase != 0 || tn.rec_soa) {
            pb::set_error("pb_lbl_extinction: %zu B of line records exceed the record budget of "
                          "%zu B and this call cannot be chunked (%s)", rec16_bytes, budget,
                          phase != 0 ? "two-phase shard call"
                                     : rounds ? "round gather" : "records are not packable");
            g.rc = PB_ERR_NOMEM;
            return g;
        }
        const int osamp = v->osamp;
        const int64_t gmax = (int64_t)(budget / ((size_t)nlayers * sizeof(Rec16)));
        Chunk c{0, 0, 0, 0};
        int64_t biggest = 0;
        for (int i = 0; i < a.niso; i++)
            for (int ph = 0; ph < osamp; ph++) {
                const int64_t g0 = p->h_ph_start[(size_t)i * (osamp + 1) + ph];
                const int64_t g1 = p->h_ph_start[(size_t)i * (osamp + 1) + ph + 1];
                if (g1 - g0 > gmax) {
                    pb::set_error("pb_lbl_extinction: the %lld groups of one (isotope, phase) key "
                                  "need more than the record budget of %zu B",
                                  (long long)(g1 - g0), budget);
                    g.rc = PB_ERR_NOMEM;
                    return g;
                }
                if (g1 - c.g_lo > gmax) {              // close the chunk before this key
                    g.chunks.push_back(c);
                    biggest = std::max(biggest, c.g_hi - c.g_lo);
                    c.key_lo = i * osamp + ph;
                    c.g_lo = g0;
                }
                c.key_hi = i * osamp + ph + 1;
                c.g_hi = g1;
            }
        g.chunks.push_back(c);
        biggest = std::max(biggest, c.g_hi - c.g_lo);
        g.rec16_need = (size_t)std::max<int64_t>(1, biggest) * nlayers * sizeof(Rec16);
    }
    g.packed = staged && !scatter && packable &&
               (g.nch_max > 1 || !g.chunks.empty() || !tn.rec_soa);
    g.fmt = scatter ? 3 : g.packed ? (g.nch_max > 1 ? 2 : 1) : 0;
    return g;
}

// Which layers are resident is decided on the device; whether the resident kernel is launched at
// all follows what the host last saw of that decision (pb_lbl::res_seen).  This is the part of
// the plan that needs the stream and the handle's counters.
static void resident_probe(pb_lbl *p, GatherPlan &g, hipStream_t s, int phase)
{
    if (!g.res_auto)
        return;
    if (phase == 2) {
        g.resident = p->res_on_pending;
        g.res_look = p->res_look_pending;
        return;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cs) == hipSuccess &&
                           cs != hipStreamCaptureStatusNone;
    const bool probe = !capturing && (p->res_seen < 0 || (p->res_calls++ & 255) == 255);
    if (!probe && p->res_seen == 0)
        g.resident = false;
    g.res_look = probe && g.resident;
    p->res_on_pending = g.resident;
    p->res_look_pending = g.res_look;
}

#ifdef PB_EXPERIMENTS
// ---------------------------------------------------------------------------
// the measured dead ends (`make EXPERIMENTS=1`) on the planner's side: the wave pair and the
// records of the scatter gather (their launches: pb_ext_gather.hip).  The default library has the
// stand-ins of the #else and of pb_ext_plan.h.
// ---------------------------------------------------------------------------
// Layers of short phase rows (<= kWvRowMax samples: the Doppler-core layers) go to the
// wave-autonomous kernel (pb_wave.hip), decided per layer on the device by k_layer_state; the
// staged kernel computes the others.  Mode 7 selects the pair; modes 0 and 2 keep to the staged
// kernel alone.  Chunked line lists continue running sums in the staged kernel's order and
// keep to it.
static void exp_wave_cap(const pb_lbl *p, LblArgs &a, const GatherPlan &g, const Tuning &tn)
{
    // (measured at C2, round 4: the pair takes 1.20 ms per extinction against 1.05 ms for the
    // staged kernel alone -- profiles/r04_gather_wave.md -- so mode 0 does not use it unless
    // PB_WAVE=1 asks for it)
    const bool can = g.staged && !g.rounds && !g.scatter && g.chunks.empty() && a.rec16 != nullptr;
    bool wave_on = can && p->gather_mode == 7;
    if (tn.wave >= 0)
        wave_on = can && (p->gather_mode == 0 || p->gather_mode == 7) && tn.wave != 0;
    if (wave_on && wave_lds(a) <= 160 * 1024)
        a.wave_cap = kWvRowMax;
}

static int exp_scatter_records(pb_lbl *p, LblArgs &a, const Tuning &tn, hipStream_t s)
{
    const size_t n = (size_t)p->max_layers * (size_t)p->lines->ngroups;
    const size_t had = p->rec32_bytes;
    if (int rc = ensure_bytes((void **)&p->rec32, &p->rec32_bytes, n * sizeof(Rec32), s, false,
                              "line records"))
        return rc;
    if (p->rec32_bytes != had) {
        PB_HIP(hipMemsetAsync(p->rec32, 0, n * sizeof(Rec32), s));
        if (tn.poison)
            k_poison_records<<<1024, kBlock, 0, s>>>(nullptr, 0, p->rec32, (int64_t)n, nullptr,
                                                    nullptr, 0);
    }
    a.rec32 = p->rec32;
    return PB_OK;
}

// the short-row layers first: many short workgroups, then the staged kernel's long ones
int exp_launch_wave(const LblArgs &a, int nunits, hipStream_t s)
{
    return a.wave_cap > 0 ? wave_launch(a, nunits, s) : PB_OK;
}
#else
static inline void exp_wave_cap(const pb_lbl *, LblArgs &, const GatherPlan &, const Tuning &) {}
static inline int exp_scatter_records(pb_lbl *, LblArgs &, const Tuning &, hipStream_t) { return PB_OK; }
#endif  // PB_EXPERIMENTS

// The record buffers the plan needs, grown on first use and bound to the arguments.  They are
// zeroed when allocated (fill_args: a record never written is a dead record).
static int bind_records(pb_lbl *p, LblArgs &a, const GatherPlan &g, const Tuning &tn, hipStream_t s)
{
    const pb_lines *l = p->lines;
    const size_t n = (size_t)p->max_layers * (size_t)l->ngroups;
    if (g.packed) {
        const size_t had = p->rec16_alloc;
        if (int rc = ensure_bytes((void **)&p->rec16, &p->rec16_alloc, g.rec16_need, s, true,
                                  "line records"))
            return rc;
        if (p->rec16_alloc != had) {
            PB_HIP(hipMemsetAsync(p->rec16, 0, g.rec16_need, s));
            if (tn.poison)
                k_poison_records<<<1024, kBlock, 0, s>>>(p->rec16, (int64_t)(g.rec16_need / sizeof(Rec16)),
                                                        nullptr, 0, nullptr, nullptr, 0);
        }
        a.rec16 = p->rec16;
    }
    exp_wave_cap(p, a, g, tn);
    if (g.scatter)
        if (int rc = exp_scatter_records(p, a, tn, s))
            return rc;
    // the SoA records serve the global gather, the resident layers and PB_REC_SOA
    const bool need_soa = g.use_records && !g.scatter && (a.rec16 == nullptr || a.res_cap > 0);
    if (need_soa && !p->rec_k) {
        size_t b0 = 0, b1 = 0;
        int rc = ensure_bytes((void **)&p->rec_k, &b0, n * 8, s, false, "line records");
        if (rc == PB_OK)
            rc = ensure_bytes((void **)&p->rec_i32, &b1, n * 4 * 5, s, false, "line records");
        if (rc)
            return rc;
        PB_HIP(hipMemsetAsync(p->rec_k, 0, n * 8, s));
        PB_HIP(hipMemsetAsync(p->rec_i32, 0, n * 4 * 5, s));
        if (tn.poison)
            k_poison_records<<<1024, kBlock, 0, s>>>(nullptr, 0, nullptr, 0, p->rec_k, p->rec_i32,
                                                    (int64_t)n);
    }
    if (g.use_records) {
        a.rec_k = p->rec_k;
        a.rec_ulo = p->rec_i32;
        a.rec_uhi = p->rec_i32 + n;
        a.rec_q = p->rec_i32 + 2 * n;
        a.rec_cell = p->rec_i32 + 3 * n;
        a.rec_phi = p->rec_i32 + 4 * n;
        // records are laid out in the order the chosen gather kernel walks the groups
        a.rk_first = g.staged ? p->ph_first : l->d_gfirst;
        a.rk_count = g.staged ? p->ph_count : l->d_gcount;
        a.rk_iown = g.staged ? p->ph_iown : l->d_giown;
        a.rk_iso = g.staged ? p->ph_iso : l->d_giso;
        const double *lead = g.staged ? p->ph_lead : p->g_lead;
        a.rk_lwn = lead;
        a.rk_elow = lead + l->ngroups;
        a.rk_gf = lead + 2 * l->ngroups;
    }
    a.use_records = g.use_records ? 1 : 0;
    return PB_OK;
}

// An out-of-core line list, chunk by chunk.
// pass 1: the per-row maxima over ALL lines (the threshold of every chunk's gather);
// pass 2: per chunk, the records of its groups, then the gather, which continues the
// running sums of the earlier chunks.  One workgroup per tile (no phase split): the sums
// of a sample are then exactly those of a single launch over every key.
static int run_chunked(pb_lbl *p, LblArgs &a, const GatherPlan &g, hipStream_t s)
{
    const int nlayers = a.nlayers;
    if (int rc = launch_kmax(a, s))
        return rc;
    const bool timed = p->ev_used + 2 <= (int)p->ev.size();
    if (timed)
        PB_HIP(hipEventRecord(p->ev[p->ev_used], s));
    const int per = kRecLayers;
    const size_t rlds = records_lds(a, per) + 8;
    PB_REQUIRE(rlds <= 64 * 1024, "pb_lbl_extinction: %zu B of LDS for the record kernel", rlds);
    a.ntiles = pb::div_up(a.wcount, g.S * kStagedSub);
    const int unit_groups = (nlayers + 7) / 8;
    dim3 ggrid((unsigned)(8 * a.ntiles * unit_groups), a.nrows);
    GatherKernel kern = staged_kernel(g.S, g.dma, a.rows_cap);
    if (int rc = allow_lds(reinterpret_cast<const void *>(kern), g.lds))
        return rc;
    for (size_t c = 0; c < g.chunks.size(); c++) {
        a.grp_lo = g.chunks[c].g_lo;
        a.grp_hi = g.chunks[c].g_hi;
        a.rec_pitch = std::max<int64_t>(1, a.grp_hi - a.grp_lo);
        a.key_lo = g.chunks[c].key_lo;
        a.key_hi = g.chunks[c].key_hi;
        a.accumulate = c > 0 ? 1 : 0;
        if (a.grp_hi > a.grp_lo) {
            dim3 rgrid(pb::div_up(a.grp_hi - a.grp_lo, kBlock), pb::div_up(nlayers, per));
            if (int rc = launch_records(a, g.fmt, per, rgrid, rlds, s))
                return rc;
        }
        kern<<<ggrid, kStagedThreads, g.lds, s>>>(a);
        PB_LAUNCH_CHECK();
    }
    p->last_gather = 2;
    p->last_args = a;
    p->last_packed = false;
    if (timed) {
        PB_HIP(hipEventRecord(p->ev[p->ev_used + 1], s));
        p->ev_used += 2;
    }
    return PB_OK;
}

// Window map of a two-phase shard call: only the groups within reach of the shard get a thread
// of k_records (LblArgs::wm_*).  Cached for the window and the walk order it was built for.
static int window_map(pb_lbl *p, LblArgs &a, bool staged, hipStream_t s)
{
    const pb_lines *l = p->lines;
    const int osamp = p->voigt->osamp, niso = a.niso;
    if (p->wm_flo != a.rec_flo || p->wm_fhi != a.rec_fhi || p->wm_staged != (int)staged) {
        const int n0 = staged ? niso * osamp : niso, n1 = niso;
        std::vector<int32_t> &h = p->h_wm;
        h.assign((size_t)2 * n0 + 1 + 2 * n1 + 1, 0);
        int32_t *lo0 = h.data(), *off0 = lo0 + n0, *lo1 = off0 + n0 + 1, *off1 = lo1 + n1;
        const int64_t flo = std::max<int64_t>(a.rec_flo, INT32_MIN);
        const int64_t fhi = std::min<int64_t>(a.rec_fhi, INT32_MAX);
        auto run = [&](const std::vector<int32_t> &pos, int64_t b, int64_t e, int32_t *lo,
                       int32_t *off, int r) {
            const auto first = pos.begin() + b, last = pos.begin() + e;
            const auto x0 = std::lower_bound(first, last, (int32_t)flo);
            const auto x1 = std::upper_bound(x0, last, (int32_t)fhi);
            lo[r] = (int32_t)(x0 - pos.begin());
            off[r + 1] = off[r] + (int32_t)(x1 - x0);
        };
        for (int i = 0; i < niso; i++) {
            run(l->h_giown, l->iso_gstart[(size_t)i], l->iso_gstart[(size_t)i + 1], lo1, off1, i);
            if (staged)
                for (int ph = 0; ph < osamp; ph++)
                    run(p->h_ph_iown, p->h_ph_start[(size_t)i * (osamp + 1) + ph],
                        p->h_ph_start[(size_t)i * (osamp + 1) + ph + 1], lo0, off0,
                        i * osamp + ph);
            else
                run(l->h_giown, l->iso_gstart[(size_t)i], l->iso_gstart[(size_t)i + 1], lo0, off0, i);
        }
        if (int rc = ensure_bytes((void **)&p->d_wm, &p->wm_bytes, h.size() * 4, s, false,
                                  "the window map"))
            return rc;
        PB_HIP(hipMemcpyAsync(p->d_wm, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
        p->wm_flo = a.rec_flo;
        p->wm_fhi = a.rec_fhi;
        p->wm_staged = (int)staged;
        p->wm_n0 = n0;
        p->wm_n1 = n1;
        p->wm_total0 = off0[n0];
        p->wm_total1 = off1[n1];
    }
    a.wm_n[0] = p->wm_n0;
    a.wm_n[1] = p->wm_n1;
    a.wm_lo[0] = p->d_wm;
    a.wm_off[0] = p->d_wm + p->wm_n0;
    a.wm_lo[1] = p->d_wm + 2 * p->wm_n0 + 1;
    a.wm_off[1] = a.wm_lo[1] + p->wm_n1;
    a.wm_total[0] = p->wm_total0;
    a.wm_total[1] = p->wm_total1;
    return PB_OK;
}

// the records (and with them the per-row maxima) of every layer of the call
static int make_records(pb_lbl *p, LblArgs &a, const GatherPlan &g, const Tuning &tn, hipStream_t s)
{
    // (one layer per thread for launches of few layers measured slower: 10 layers of C2
    // 49 us against 27 us with four -- kRecLayers was 4 then; PB_REC_LAYERS=1 selects it)
    const int per = tn.rec_layers_1 ? 1 : kRecLayers;
    int64_t rec_threads = a.ngroups;
    if (a.kmax_local && a.rec_flo != INT64_MIN && !p->h_ph_iown.empty() && !tn.no_window_map) {
        if (int rc = window_map(p, a, g.staged, s))
            return rc;
        rec_threads = std::max<int64_t>(1, std::max(p->wm_total0, p->wm_total1));
    }
    dim3 grid(pb::div_up(rec_threads, kBlock), pb::div_up(a.nlayers, per));
    // the run offsets of the phase-order window map go to LDS while they fit beside the rest
    // in 48 KiB (niso * osamp + 1 words: the reference's default wnosamp of 2160 with 8
    // isotopes is already 69 KiB); larger maps are bisected in global memory
    const size_t rlds0 = records_lds(a, per);
    const size_t wm_bytes = ((size_t)a.wm_n[0] + 2) * 4;
    a.wm_lds = a.wm_off[0] && rlds0 + wm_bytes <= tn.wm_lds_cap ? 1 : 0;
    const size_t rlds = rlds0 + (a.wm_lds ? wm_bytes : 8);
    PB_REQUIRE(rlds <= 64 * 1024, "pb_lbl_extinction: %zu B of LDS for the record kernel "
               "(too many isotopes / output rows)", rlds);
    return launch_records(a, g.fmt, per, grid, rlds, s);
}

// what the call leaves in the handle: the resident decision (when this call looks), the
// arguments for pb_lbl_last_work, the end of the timed span
static int finish_call(pb_lbl *p, const LblArgs &a, bool res_look, bool timed, hipStream_t s)
{
    if (res_look) {
        std::vector<int32_t> h((size_t)a.nlayers);
        PB_HIP(hipMemcpyAsync(h.data(), p->ls_resident, (size_t)a.nlayers * 4, hipMemcpyDeviceToHost, s));
        PB_HIP(hipStreamSynchronize(s));
        p->res_seen = std::any_of(h.begin(), h.end(), [](int32_t v) { return v != 0; }) ? 1 : 0;
    }
    p->last_args = a;
    // (chunked records are counted only in the one-row form with every isotope kept: the entries
    // of a skipped isotope are never written)
    p->last_packed = a.rec16 != nullptr &&
                     (a.nch_max == 1 ||
                      (a.nrows == 1 && std::all_of(p->isoiext.begin(), p->isoiext.end(),
                                                   [](int32_t v) { return v >= 0; })));
    if (timed) {
        PB_HIP(hipEventRecord(p->ev[p->ev_used + 1], s));
        p->ev_used += 2;
    }
    return PB_OK;
}

// phase 0: the whole call; 1: up to and including the records, per-row maxima over the shard's
// own groups only (the caller all-reduces them); 2: the gather of the call begun with phase 1
int lbl_extinction(pb_lbl *p, const Call &c, void *stream, int phase)
{
    PB_REQUIRE(p, "pb_lbl_extinction: null handle");
    PB_REQUIRE(c.wcount == 0 || (c.ext && c.temp && c.dens && c.isoz),
               "pb_lbl_extinction: null pointer");
    PB_REQUIRE(c.nlayers >= 1 && c.nlayers <= p->max_layers,
               "pb_lbl_extinction: nlayers=%d outside [1,%d]", c.nlayers, p->max_layers);
    PB_REQUIRE(c.wbegin >= 0 && c.wcount >= 0 && c.wbegin + c.wcount <= p->nwave,
               "pb_lbl_extinction: shard [%lld,+%lld) outside the %d-sample grid",
               (long long)c.wbegin, (long long)c.wcount, p->nwave);
    hipStream_t s = pb::as_stream(stream);
    if (c.wcount == 0) {
        // an empty shard of a two-phase call still takes part in the all-reduce(MAX) of the
        // per-row maxima: it must contribute zeros, not what its previous call left behind
        if (phase == 1)
            PB_HIP(hipMemsetAsync(p->kmax_bits, 0, (size_t)p->max_layers * p->kmax_rows * 8, s));
        return PB_OK;
    }
    const pb_lines *l = p->lines;
    if (p->resolution)
        if (int rc = pb_voigt_ensure_flat(p->voigt, s))
            return rc;
    const Tuning tn = read_tuning();
    LblArgs a = fill_args(p, c);
    a.kmax_local = phase != 0 ? 1 : 0;
    a.experiment = tn.experiment;

    GatherPlan g = plan_gather(p, a, tn, phase);
    resident_probe(p, g, s, phase);
    if (g.rc)
        return g.rc;
    const bool chunked = !g.chunks.empty();
    p->last_chunks = (int)g.chunks.size();
    a.nch_max = g.nch_max;
    a.rowlds = g.rowlds;
    // rows per barrier step of the staged gather: stage_slots() up to this cap on the LDS-DMA
    // path with rows in one piece, one row per step otherwise (PB_STAGE_ROWS=1: everywhere)
    // (the launches of a dynamic-grid sub-plan: one unless PB_STAGE_ROWS says otherwise)
    a.rows_cap = g.dma && g.nch_max == 1
                     ? (tn.stage_rows ? tn.stage_rows : p->dyn_child ? 1 : kStageRowsDefault)
                     : 1;
    a.res_cap = g.resident && !chunked ? p->res_cap : 0;   // (chunked: every layer through the staged gather)
    if (int rc = bind_records(p, a, g, tn, s))
        return rc;

    bool dyn_fall = false;
    // (a fine grid shorter than two steps of the coarsest dynamic grid has no constant-step form)
    if (p->resolution && p->gather_mode == 6 && phase == 0 && l->ngroups > 0 &&
        l->onwn > 2 * (int64_t)p->voigt->osamp && !tn.res_dyn_off) {
        const int rc = lbl_resolution_dyn(p, a, c, tn, s);
        // a re-cut table row that cannot be addressed (pb_voigt_ensure_rows) before any run has
        // added to ext: the direct gather below computes the call instead
        if (!(rc == PB_ERR_UNSUPPORTED && p->dyn_runs == 0)) {
            if (rc != PB_OK || !p->dyn_fallback)
                return rc;
            // a call planned from a prediction: the layers the plan did not fit (none, as a
            // rule: the launches below then end at once) go through the direct gather
            dyn_fall = true;
            a.lskip = p->d_ok;
        }
    }
    if (phase != 2 && !dyn_fall)
        if (int rc = launch_layer_state(a, s))
            return rc;
    if (chunked)
        return run_chunked(p, a, g, s);
    int rc = PB_OK;
    if (phase != 2)                      // (phase 2: records and maxima are in place)
        rc = g.use_records ? make_records(p, a, g, tn, s) : l->nlines > 0 ? launch_kmax(a, s) : PB_OK;
    if (rc || phase == 1)
        return rc;

    const bool timed = !dyn_fall && p->ev_used + 2 <= (int)p->ev.size();
    if (timed)
        PB_HIP(hipEventRecord(p->ev[p->ev_used], s));
    p->last_gather = dyn_fall ? 6 : g.scatter ? 4
                             : (p->resolution ? 3 : g.rounds ? 5 : g.staged ? 2 : 1) +
                                   (g.resident ? 8 : 0) + (a.wave_cap > 0 ? 16 : 0);
    if (g.scatter) {                     // (computes every layer)
        rc = exp_launch_scatter(a, tn, s);
    } else {
        // the layers with narrow profiles, then the others
        if (g.resident)
            rc = launch_resident(a, s);
        if (rc == PB_OK)
            rc = p->resolution ? launch_linterp(a, s)
                 : g.rounds    ? exp_launch_rounds(p, a, g, tn, s)
                 : g.staged    ? launch_staged(p, a, g, tn, s)
                               : launch_global(a, tn, s);
    }
    if (rc)
        return rc;
    return finish_call(p, a, g.res_look, timed, s);
}

}  // namespace pbx

extern "C" {

int pb_lbl_extinction(pb_lbl *p, double *ext_d, int64_t wbegin, int64_t wcount,
                      const double *temp_d, const double *dens_d, const double *isoz_d,
                      int64_t z_iso_stride, int64_t z_layer_stride, int nlayers, int add,
                      void *stream)
{
    const Call c{ext_d, wbegin, wcount, temp_d, dens_d, isoz_d, z_iso_stride, z_layer_stride,
                 nlayers, add, false};
    return lbl_extinction(p, c, stream, 0);
}

int pb_lbl_extinction_begin(pb_lbl *p, double *ext_d, int64_t wbegin, int64_t wcount,
                            const double *temp_d, const double *dens_d, const double *isoz_d,
                            int64_t z_iso_stride, int64_t z_layer_stride, int nlayers, int add,
                            void *stream)
{
    PB_REQUIRE(p, "pb_lbl_extinction_begin: null handle");
    p->pending = {ext_d, wbegin, wcount, temp_d, dens_d, isoz_d, z_iso_stride, z_layer_stride,
                  nlayers, add, true};
    return lbl_extinction(p, p->pending, stream, 1);
}

int pb_lbl_extinction_end(pb_lbl *p, void *stream)
{
    PB_REQUIRE(p && p->pending.open, "pb_lbl_extinction_end: no call was begun");
    p->pending.open = false;
    return lbl_extinction(p, p->pending, stream, 2);
}

int pb_lbl_kmax_buffer(pb_lbl *p, void **kmax_d, int64_t *count)
{
    PB_REQUIRE(p && kmax_d && count, "pb_lbl_kmax_buffer: null pointer");
    *kmax_d = p->kmax_bits;
    *count = (int64_t)p->max_layers * p->kmax_rows;
    return PB_OK;
}

int pb_lbl_timing_begin(pb_lbl *p, int max_launches)
{
    PB_REQUIRE(p && max_launches >= 0, "pb_lbl_timing_begin: bad argument");
    while ((int)p->ev.size() < 2 * max_launches) {
        hipEvent_t e;
        PB_HIP(hipEventCreate(&e));
        p->ev.push_back(e);
    }
    while ((int)p->ev.size() > 2 * max_launches) {
        (void)hipEventDestroy(p->ev.back());
        p->ev.pop_back();
    }
    p->ev_used = 0;
    return PB_OK;
}

int pb_lbl_timing_end(pb_lbl *p, double *total_ms, int *launches)
{
    PB_REQUIRE(p && total_ms && launches, "pb_lbl_timing_end: null pointer");
    double sum = 0.0;
    for (int i = 0; i + 1 < p->ev_used; i += 2) {
        PB_HIP(hipEventSynchronize(p->ev[i + 1]));
        float ms = 0.f;
        PB_HIP(hipEventElapsedTime(&ms, p->ev[i], p->ev[i + 1]));
        sum += ms;
    }
    *total_ms = sum;
    *launches = p->ev_used / 2;
    p->ev_used = 0;
    for (hipEvent_t e : p->ev)
        (void)hipEventDestroy(e);
    p->ev.clear();
    return PB_OK;
}

int pb_lbl_last_state(pb_lbl *p, int32_t *ofactor_h, double *kmax_h, int nlayers, int nrows,
                      void *stream)
{
    PB_REQUIRE(p, "pb_lbl_last_state: null handle");
    PB_REQUIRE(nlayers >= 1 && nlayers <= p->max_layers && nrows >= 1 && nrows <= p->kmax_rows,
               "pb_lbl_last_state: bad sizes");
    PB_HIP(hipStreamSynchronize(pb::as_stream(stream)));
    if (ofactor_h)
        PB_HIP(hipMemcpy(ofactor_h, p->ls_ofactor, (size_t)nlayers * 4, hipMemcpyDeviceToHost));
    if (kmax_h)
        PB_HIP(hipMemcpy(kmax_h, p->kmax_bits, (size_t)nlayers * nrows * 8,
                         hipMemcpyDeviceToHost));
    return PB_OK;
}

int pb_lbl_last_layer_kinds(pb_lbl *p, int32_t *resident_h, int32_t *block_h, int nlayers,
                            void *stream)
{
    PB_REQUIRE(p, "pb_lbl_last_layer_kinds: null handle");
    PB_REQUIRE(nlayers >= 1 && nlayers <= p->max_layers, "pb_lbl_last_layer_kinds: bad sizes");
    PB_HIP(hipStreamSynchronize(pb::as_stream(stream)));
    if (resident_h)
        PB_HIP(hipMemcpy(resident_h, p->ls_resident, (size_t)nlayers * 4, hipMemcpyDeviceToHost));
    if (block_h)
        PB_HIP(hipMemcpy(block_h, p->ls_block, (size_t)nlayers * 4, hipMemcpyDeviceToHost));
    return PB_OK;
}

int pb_lbl_rows_per_step(int rowlds, int rowlim, int *pitch)
{
    const StageSlots sl = stage_slots(rowlds, rowlim);
    if (pitch)
        *pitch = sl.pitch;
    return sl.rows;
}

int pb_lbl_last_rows_per_step(pb_lbl *p, int32_t *rows_h, int nlayers, int niso, void *stream)
{
    PB_REQUIRE(p && rows_h, "pb_lbl_last_rows_per_step: null pointer");
    PB_REQUIRE(nlayers >= 1 && nlayers <= p->max_layers && niso == p->niso,
               "pb_lbl_last_rows_per_step: bad sizes");
    PB_HIP(hipStreamSynchronize(pb::as_stream(stream)));
    const size_t n = (size_t)nlayers * niso;
    const LblArgs &a = p->last_args;
    if ((p->last_gather & 7) != 2 || a.rows_cap <= 1) {       // not the staged gather, or one row per step
        std::fill(rows_h, rows_h + n, 1);
        return PB_OK;
    }
    PB_HIP(hipMemcpy(rows_h, p->li_rowmax, n * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)
        rows_h[i] = stage_slots(a.rowlds, std::min(a.rowlds, rows_h[i]), a.rows_cap).rows;
    return PB_OK;
}

#ifdef PB_EXPERIMENTS
int pb_lbl_last_wave_layers(pb_lbl *p, int32_t *wave_h, int nlayers, void *stream)
{
    PB_REQUIRE(p && wave_h, "pb_lbl_last_wave_layers: null pointer");
    PB_REQUIRE(nlayers >= 1 && nlayers <= p->max_layers, "pb_lbl_last_wave_layers: bad sizes");
    PB_HIP(hipStreamSynchronize(pb::as_stream(stream)));
    if (p->last_args.wave_cap > 0)
        PB_HIP(hipMemcpy(wave_h, p->ls_wave, (size_t)nlayers * 4, hipMemcpyDeviceToHost));
    else
        memset(wave_h, 0, (size_t)nlayers * 4);
    return PB_OK;
}

#endif  // PB_EXPERIMENTS

void pb_lbl_destroy(pb_lbl *p)
{
    if (!p)
        return;
    (void)hipFree(p->d_wn);
    (void)hipFree(p->d_molrad);
    (void)hipFree(p->d_molmass);
    (void)hipFree(p->d_isomass);
    (void)hipFree(p->d_isoratio);
    (void)hipFree(p->d_divisors);
    (void)hipFree(p->d_isoimol);
    (void)hipFree(p->d_isoiext);
    (void)hipFree(p->ls_ofactor);
    (void)hipFree(p->ls_scale);
    (void)hipFree(p->ls_resident);
    (void)hipFree(p->ls_block);
    (void)hipFree(p->ls_wave);
    (void)hipFree(p->d_tsplit);
    (void)hipFree(p->pos2ph);
    (void)hipFree(p->rec32);
    (void)hipFree(p->rec16);
    (void)hipFree(p->part);
    (void)hipFree(p->d_wm);
    (void)hipFree(p->d_unit_tab);
    (void)hipFree(p->d_lsplit);
    (void)hipFree(p->gs_start);
    (void)hipFree(p->ls_dnwn);
    (void)hipFree(p->ls_dwnstep);
    (void)hipFree(p->ls_quot);
    (void)hipFree(p->li_alphad);
    (void)hipFree(p->li_dens);
    (void)hipFree(p->li_z);
    (void)hipFree(p->li_invz);
    (void)hipFree(p->li_ilor);
    (void)hipFree(p->li_hmax);
    (void)hipFree(p->li_rowmax);
    (void)hipFree(p->li_hlo);
    (void)hipFree(p->li_hhi);
    (void)hipFree(p->kmax_bits);
    (void)hipFree(p->unit_cap);
    (void)hipFree(p->vrec);
    (void)hipFree(p->vseg);
    (void)hipFree(p->vrnd);
    (void)hipFree(p->uhdr);
    (void)hipFree(p->ph_first);
    (void)hipFree(p->ph_count);
    (void)hipFree(p->ph_iown);
    (void)hipFree(p->ph_start);
    (void)hipFree(p->ph_iso);
    (void)hipFree(p->ph_bin);
    (void)hipFree(p->ph_lead);
    (void)hipFree(p->g_lead);
    (void)hipFree(p->rec_k);
    (void)hipFree(p->rec_i32);
    for (hipEvent_t e : p->ev)
        (void)hipEventDestroy(e);
    for (pb_lbl::DynSub &d : p->dyn) {
        pb_lbl_destroy(d.plan);                        // (their tables belong to p->voigt)
        (void)hipFree(d.ktmp);
    }
    for (hipStream_t t : p->dyn_streams)
        (void)hipStreamDestroy(t);
    for (hipEvent_t e : p->dyn_join)
        (void)hipEventDestroy(e);
    if (p->dyn_fork)
        (void)hipEventDestroy(p->dyn_fork);
    if (p->rb_ev)
        (void)hipEventDestroy(p->rb_ev);
    (void)hipFree(p->d_pred_f);
    (void)hipFree(p->d_ok);
    (void)hipFree((void *)p->d_pred_mask);
    if (p->rb_host)
        (void)hipHostFree(p->rb_host);
    delete p;
}

static int interp_ec_launch(bool assign, double *extinction_d, const double *etable_d,
                            const double *ttable_d, const double *temperatures_d,
                            const double *density_d, int nmol, int ntemp, int nlayers,
                            int nwave, int lay1, int lay2, int per_mol, void *stream)
{
    PB_REQUIRE(nmol >= 1 && ntemp >= 2 && nlayers >= 1 && nwave >= 0,
               "pb_interp_ec: bad shape (needs >= 2 table temperatures)");
    PB_REQUIRE(lay1 >= 0, "pb_interp_ec: lay1 < 0");
    if (lay2 > nlayers)
        lay2 = nlayers;
    if (lay2 <= lay1 || nwave == 0)
        return PB_OK;
    PB_REQUIRE(extinction_d && etable_d && ttable_d && temperatures_d && density_d,
               "pb_interp_ec: null pointer");
    dim3 grid(pb::div_up(nwave, kBlock), lay2 - lay1, per_mol ? nmol : 1);
    if (assign)
        k_interp_ec<true><<<grid, kBlock, 0, pb::as_stream(stream)>>>(
            extinction_d, etable_d, ttable_d, temperatures_d, density_d, nmol, ntemp, nlayers,
            nwave, lay1, per_mol ? 1 : 0);
    else
        k_interp_ec<false><<<grid, kBlock, 0, pb::as_stream(stream)>>>(
            extinction_d, etable_d, ttable_d, temperatures_d, density_d, nmol, ntemp, nlayers,
            nwave, lay1, per_mol ? 1 : 0);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_interp_ec(double *extinction_d, const double *etable_d, const double *ttable_d,
                 const double *temperatures_d, const double *density_d, int nmol, int ntemp,
                 int nlayers, int nwave, int lay1, int lay2, int per_mol, void *stream)
{
    return interp_ec_launch(false, extinction_d, etable_d, ttable_d, temperatures_d, density_d,
                            nmol, ntemp, nlayers, nwave, lay1, lay2, per_mol, stream);
}

int pb_interp_ec_set(double *extinction_d, const double *etable_d, const double *ttable_d,
                     const double *temperatures_d, const double *density_d, int nmol, int ntemp,
                     int nlayers, int nwave, int lay1, int lay2, int per_mol, void *stream)
{
    return interp_ec_launch(true, extinction_d, etable_d, ttable_d, temperatures_d, density_d,
                            nmol, ntemp, nlayers, nwave, lay1, lay2, per_mol, stream);
}

}  // extern "C"
