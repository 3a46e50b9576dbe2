// Line-by-line extinction, step 3 of the launch sequence (pb_extinction.hip) for `resolution`
// plans: the direct gather on an arbitrary output grid (k_ext_linterp) and gather mode 6, the
// per-layer dynamic grids computed by constant-step sub-plans (lbl_resolution_dyn), with the
// predicted run plans of the experiments build.
#include <algorithm>
#include <vector>

#include "pb_ext_plan.h"

using namespace pbx;

namespace {

// ---------------------------------------------------------------------------
// 3b. gather, arbitrary output grid (resolution / wlstep mode): every output needs the
// two dynamic-grid samples that bracket it (linterp, utils.h:139-163).  Uses the
// reference-layout table (the stride between consecutive outputs is not constant).
// One output sample per lane, 256 per workgroup.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ext_linterp(LblArgs a)
{
    // one record of the batch: two 16-byte LDS broadcast reads per (record, wavefront)
    struct __align__(16) RecA {
        double k;
        int64_t start;                                  // start of the profile in flat[]
    };
    struct __align__(16) RecB {
        int inoff, half2, mn, mx;                       // half - iown, 2*half, window [mn, mx)
    };
    __shared__ RecA s_ra[kBlock + 4];
    __shared__ RecB s_rb[kBlock + 4];

    int tile, layer;
    decode_block(a, tile, layer);
    if (layer < 0)
        return;
    if (a.lskip && uniform_load_i32(a.lskip, layer))
        return;
    const int row = blockIdx.y;

    const int64_t t0 = a.wbegin + (int64_t)tile * kBlock;
    const int64_t tend = min(t0 + kBlock, a.wbegin + a.wcount);
    const int64_t jo = t0 + threadIdx.x;
    const bool live = jo < tend;

    const int ofactor = a.ls_ofactor[layer];
    const int64_t dnwn = a.ls_dnwn[layer];
    const double dwnstep = a.ls_dwnstep[layer];
    const double temp = a.temp[layer];
    const double kthresh =
        a.ethresh * __longlong_as_double((long long)a.kmax_bits[(int64_t)layer * a.nrows + row]);

    // bracketing dynamic-grid sample of this output and of the tile's ends
    const double wn_i = live ? a.wn[jo] : a.wn[tend - 1];
    const int ilo = (int)((wn_i - a.wn0) / dwnstep);
    const int tile_jmin = (int)((a.wn[t0] - a.wn0) / dwnstep);
    const int tile_jmax = (int)((a.wn[tend - 1] - a.wn0) / dwnstep) + 1;

    double acc0 = 0.0, acc1 = 0.0;
    for (int iso = 0; iso < a.niso; iso++) {
        const int iext = a.isoiext[iso];
        if (iext < 0 || (a.add ? 0 : iext) != row)
            continue;
        const int64_t li = (int64_t)layer * a.niso + iso;
        const int ilor = a.li_ilor[li];
        const double alphad = a.li_alphad[li];
        const double ratio = a.isoratio[iso];
        const double z = a.li_z[li], inv_z = a.li_invz[li];
        const double inv_temp = a.ls_inv_temp[layer];
        const double dens = a.li_dens[li];
        int64_t reach = a.li_hmax[li];
        if (a.cutoff > 0.0)
            reach = min(reach, (int64_t)(a.cutoff / a.ownstep) + 2 * (int64_t)ofactor + 2);
        reach += 2 * (int64_t)ofactor;
        const int64_t seg0 = a.iso_gstart[iso], seg1 = a.iso_gstart[iso + 1];
        const int64_t g0 =
            lower_bound_i32(a.giown, seg0, seg1, (int64_t)tile_jmin * ofactor - reach);
        const int64_t g1 =
            lower_bound_i32(a.giown, seg0, seg1, (int64_t)tile_jmax * ofactor + reach + 1);
        for (int64_t gb = g0; gb < g1; gb += kBlock) {
            __syncthreads();
            {
                const int64_t g = gb + threadIdx.x;
                double k = 0.0;
                int64_t start = 0;
                int mn = 0, mx = 0, half2 = 0, inoff = 0;
                if (g < g1) {
                    const int first = a.gfirst[g];
                    const int iown = a.giown[g];
                    k = group_strength(a, first, a.gcount[g], ratio, temp, inv_temp, z, inv_z);
                    if (!(k < kthresh)) {
                        if (a.add)
                            k *= dens;
                        const Window w = group_window(a, a.lwn[first], iown, ilor, alphad,
                                                      ofactor, dwnstep, dnwn, 0, a.ndop - 1,
                                                      nullptr, a.ls_cutsteps[layer],
                                                      a.ls_inv_ofactor[layer]);
                        // dynamic sample j reads flat[pindex + half + ofactor*j - iown]
                        mn = (int)w.minj;
                        mx = (int)w.maxj;
                        half2 = 2 * w.half;
                        inoff = w.half - iown;
                        start = a.pindex[w.cell];
                    }
                }
                // (a dead record keeps an empty window, k = 0 and the start of the table)
                s_ra[threadIdx.x] = RecA{k, start};
                s_rb[threadIdx.x] = RecB{inoff, half2, mn, mx};
                if (threadIdx.x < 4) {                  // the padding of the last trip of four
                    s_ra[kBlock + threadIdx.x] = RecA{0.0, 0};
                    s_rb[kBlock + threadIdx.x] = RecB{0, 0, 0, 0};
                }
            }
            __syncthreads();
            const int nrec = (int)min((int64_t)kBlock, g1 - gb);
            // Four records per trip and NO branch around the table reads: a lane outside a
            // record's window reads element 0 of that profile with a zero strength instead.
            // Behind per-record branches every pair of reads was drained (s_waitcnt vmcnt(0))
            // before the next record's were issued; now eight gathers are in flight per lane.
            // The sums see the same terms in the same order (+ k * 0-weight terms that are
            // exactly zero: profile samples are finite).
            for (int e = 0; e < nrec; e += 4) {
                double k0[4], k1[4], v0[4], v1[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const RecA ra = s_ra[e + u];        // (entries beyond nrec: k = 0 records of
                    const RecB rb = s_rb[e + u];        // this or an earlier batch, or the padding)
                    const bool have = e + u < nrec;
                    const int64_t f0 = rb.inoff + (int64_t)ofactor * ilo;
                    const int64_t f1 = f0 + ofactor;
                    const bool in0 = have && live && ilo >= rb.mn && ilo < rb.mx && f0 >= 0 &&
                                     f0 <= rb.half2;
                    const bool in1 = have && live && ilo + 1 >= rb.mn && ilo + 1 < rb.mx && f1 >= 0 &&
                                     f1 <= rb.half2;
                    const double *tab = a.flat + ra.start;
                    v0[u] = tab[in0 ? f0 : 0];
                    v1[u] = tab[in1 ? f1 : 0];
                    k0[u] = in0 ? ra.k : 0.0;
                    k1[u] = in1 ? ra.k : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    acc0 = fma(k0[u], v0[u], acc0);
                    acc1 = fma(k1[u], v1[u], acc1);
                }
            }
        }
    }
    if (live) {
        const double wnlo = a.wn0 + dwnstep * ilo;
        a.ext[((int64_t)layer * a.nrows + row) * a.wcount + (jo - a.wbegin)] +=
            (acc0 * (wnlo + dwnstep - wn_i) + acc1 * (wn_i - wnlo)) / dwnstep;
    }
}

// 3b'. `resolution` mode through the dynamic grids: the sums of a run of layers on their
// dynamic grid (ktmp[layer][row][d0 .. d0+dcount), computed by a constant-step plan of step
// ofactor) interpolated onto the output grid exactly as utils.h:139-163 does, accumulated into ext.
// grid (output blocks, layers of the run x rows)
__global__ __launch_bounds__(kBlock) void k_dyn_interp(double *ext, const double *ktmp,
                                                      const double *wn, double wn0,
                                                      const double *dwnstep, int64_t d0,
                                                      int64_t dcount, int64_t wbegin,
                                                      int64_t wcount, int nrows,
                                                      const int32_t *ok)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= wcount)
        return;
    const int lr = blockIdx.y;
    if (!uniform_load_i32(ok, lr / nrows))               // (a layer the run plan did not fit)
        return;
    const double step = dwnstep[lr / nrows];
    const double wn_i = wn[wbegin + j];
    const int64_t ilo = (int)((wn_i - wn0) / step);
    const double *src = ktmp + (int64_t)lr * dcount - d0;
    const double v0 = ilo >= d0 && ilo < d0 + dcount ? src[ilo] : 0.0;
    const double v1 = ilo + 1 >= d0 && ilo + 1 < d0 + dcount ? src[ilo + 1] : 0.0;
    const double wnlo = wn0 + step * ilo;
    ext[(int64_t)lr * wcount + j] += (v0 * (wnlo + step - wn_i) + v1 * (wn_i - wnlo)) / step;
}

// Which layers does the run plan of a host-free `resolution` call fit?  The plan was made from
// the factors and Lorentz rows the layers had when they were last read back; a layer is computed
// by its run iff its factor is the predicted one and every Lorentz row its isotopes select is
// filled in the re-cut table of that factor (unfilled rows read as zeros: wrong, never a fault).
__global__ void k_dyn_check(int32_t *ok, const int32_t *ofactor, const int32_t *ilor,
                            const int32_t *pred_f, const uint8_t *const *pred_mask, int nlayers,
                            int niso)
{
    const int layer = blockIdx.x * blockDim.x + threadIdx.x;
    if (layer >= nlayers)
        return;
    bool good = ofactor[layer] == pred_f[layer];
    const uint8_t *mask = pred_mask[layer];
    for (int i = 0; i < niso; i++)
        good = good && mask[ilor[(int64_t)layer * niso + i]] != 0;
    ok[layer] = good ? 1 : 0;
}

// the per-row maxima of a run's layers -> the plan's (only the layers the run computed)
__global__ void k_dyn_kmax(unsigned long long *dst, const unsigned long long *src,
                           const int32_t *ok, int nl, int nrows)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nl * nrows && ok[e / nrows])
        dst[e] = src[e];
}

}  // namespace

namespace pbx {

int launch_linterp(LblArgs &a, hipStream_t s)
{
    a.ntiles = pb::div_up(a.wcount, kBlock);
    dim3 grid((unsigned)(8 * a.ntiles * ((a.nlayers + 7) / 8)), a.nrows);
    k_ext_linterp<<<grid, kBlock, 0, s>>>(a);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

// `resolution` plans, gather mode 6.  The reference accumulates every line of a layer on the
// layer's dynamic grid -- constant step, ofactor fine samples (_extcoeff.c:185-195, 281-307) -- and
// interpolates the outputs from it (:320-326).  That grid is a constant-step output grid with
// oversampling factor ofactor and nothing to resample, so a constant-step plan per factor computes
// it with the staged kernels (phase rows modulo the factor, shared in LDS by every line of a
// phase), and k_dyn_interp finishes.  Layers are walked in runs of equal factor.  The factors are
// read back from the device (one stream synchronisation per call).
static int dyn_subplan(pb_lbl *p, int f, hipStream_t s, pb_lbl::DynSub **out)
{
    for (pb_lbl::DynSub &d : p->dyn)
        if (d.f == f) {
            *out = &d;
            return PB_OK;
        }
    const pb_lines *l = p->lines;
    pb_lbl::DynSub d{f, nullptr, nullptr, nullptr, 0, 0, 0};
    int rc = pb_voigt_rephase(&d.voigt, p->voigt, f, s);
    if (rc)
        return rc;
    std::vector<int32_t> divs;
    for (int32_t x : p->h_divisors)
        if (x <= f && f % x == 0)
            divs.push_back(x);
    const int64_t dn = 1 + (l->onwn - 1) / f;
    std::vector<double> wn((size_t)dn);
    for (int64_t i = 0; i < dn; i++)
        wn[(size_t)i] = l->own0 + (double)(i * f) * l->ownstep;
    rc = pb_lbl_create(&d.plan, d.voigt, p->lines, wn.data(), (int)dn, divs.data(),
                       (int)divs.size(), p->h_molrad.data(), p->h_molmass.data(), p->nmol,
                       p->h_isoimol.data(), p->h_isomass.data(), p->h_isoratio.data(),
                       p->h_isoiext0.data(), p->niso, p->cutoff, p->ethresh, 0, p->max_layers);
    if (rc)
        return rc;                                     // (the table stays with p->voigt)
    // runs of one or two deep layers are small launches: the automatic choice would send them
    // to the global gather (c2-res: 180-580 us per layer against 55-200 staged)
    if (!getenv("PB_GATHER"))
        d.plan->gather_mode = 2;
    d.plan->dyn_child = true;
    p->dyn.push_back(d);
    *out = &p->dyn.back();
    return PB_OK;
}

int lbl_resolution_dyn(pb_lbl *p, LblArgs &a, const Call &c, const Tuning &tn, hipStream_t s)
{
    const pb_lines *l = p->lines;
    const int nlayers = c.nlayers;
    const int64_t wbegin = c.wbegin, wcount = c.wcount;
    PB_REQUIRE(l->onwn < (1LL << 30), "pb_lbl_extinction: fine grid of %lld samples exceeds 2^30",
               (long long)l->onwn);
    if (int rc = launch_layer_state(a, s))
        return rc;
    const size_t nstate = (size_t)nlayers * (1 + p->niso);
    // a finished read-back of an earlier call: adopt it as the prediction; if it contradicts the
    // prediction that call was planned with, the atmosphere is moving -- synchronise for a while
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &capturing) != hipSuccess)
        (void)hipGetLastError();
    if (capturing != hipStreamCaptureStatusNone) {
        // (no event query while a graph is being captured)
    } else if (p->rb_pending && hipEventQuery(p->rb_ev) == hipSuccess) {
        p->rb_pending = false;
        if (p->rb_layers == nlayers && p->pred_layers == nlayers) {
            const int32_t *f = p->rb_host, *il = p->rb_host + nlayers;
            const bool same_f = std::equal(f, f + nlayers, p->used_f.begin());
            if (!same_f || !std::equal(il, il + (size_t)nlayers * p->niso, p->pred_ilor.begin())) {
                p->pred_f.assign(f, f + nlayers);
                p->pred_ilor.assign(il, il + (size_t)nlayers * p->niso);
                p->pred_dirty = true;
            }
            if (!same_f) {
                p->dyn_mispredicted++;
                p->dyn_hold = 8;
            }
        }
    } else if (p->rb_pending) {
        (void)hipGetLastError();                          // (hipErrorNotReady is not an error)
    }
    // (a captured call cannot synchronise: it is planned from the prediction or not at all)
    // (the default library has no switch for it: pb_lbl_set_dyn_predict exists in the experiments
    // build only -- measured no faster)
    const bool spec = kExp && p->dyn_predict && p->pred_layers == nlayers &&
                      (capturing != hipStreamCaptureStatusNone || p->dyn_hold == 0);
    PB_REQUIRE(spec || capturing == hipStreamCaptureStatusNone,
               "pb_lbl_extinction: a `resolution` plan in gather mode 6 can be captured into a "
               "graph only with pb_lbl_set_dyn_predict(plan, 1) and after one spectrum of this "
               "many layers");
    p->h_ofactor.resize((size_t)nlayers);
    p->h_ilor.resize((size_t)nlayers * p->niso);
    if (!spec) {
        PB_HIP(hipMemcpyAsync(p->h_ofactor.data(), p->ls_ofactor, (size_t)nlayers * 4,
                              hipMemcpyDeviceToHost, s));
        PB_HIP(hipMemcpyAsync(p->h_ilor.data(), p->li_ilor, (size_t)nlayers * p->niso * 4,
                              hipMemcpyDeviceToHost, s));
        PB_HIP(hipStreamSynchronize(s));
        if (p->pred_layers != nlayers || p->pred_f != p->h_ofactor || p->pred_ilor != p->h_ilor) {
            p->pred_f = p->h_ofactor;
            p->pred_ilor = p->h_ilor;
            p->pred_layers = nlayers;
            p->pred_dirty = true;
        }
        if (p->dyn_hold > 0)
            p->dyn_hold--;
        p->dyn_sync_calls++;
    } else {
        p->h_ofactor = p->pred_f;
        p->h_ilor = p->pred_ilor;
        p->dyn_spec_calls++;
        if (!p->rb_pending && capturing == hipStreamCaptureStatusNone) {
            if (nstate > p->rb_cap) {
                if (p->rb_host)
                    (void)hipHostFree(p->rb_host);
                p->rb_host = nullptr;
                p->rb_cap = 0;
                PB_HIP(hipHostMalloc((void **)&p->rb_host, nstate * 4, hipHostMallocDefault));
                p->rb_cap = nstate;
            }
            if (!p->rb_ev)
                PB_HIP(hipEventCreateWithFlags(&p->rb_ev, hipEventDisableTiming));
            PB_HIP(hipMemcpyAsync(p->rb_host, p->ls_ofactor, (size_t)nlayers * 4,
                                  hipMemcpyDeviceToHost, s));
            PB_HIP(hipMemcpyAsync(p->rb_host + nlayers, p->li_ilor, (size_t)nlayers * p->niso * 4,
                                  hipMemcpyDeviceToHost, s));
            PB_HIP(hipEventRecord(p->rb_ev, s));
            p->rb_pending = true;
            p->rb_layers = nlayers;
        }
    }
    p->used_f = p->h_ofactor;                             // (what this call is planned with)
    p->dyn_fallback = spec;
    // every sub-plan and Lorentz row of the plan exists before the device check runs; then the
    // prediction (factor and row mask of the factor's table, per layer) goes to the device
    for (int l0 = 0; l0 < nlayers;) {
        const int f = p->h_ofactor[(size_t)l0];
        int l1 = l0 + 1;
        while (l1 < nlayers && p->h_ofactor[(size_t)l1] == f)
            l1++;
        pb_lbl::DynSub *sub = nullptr;
        int rc = dyn_subplan(p, f, s, &sub);
        if (rc)
            return rc;
        std::vector<int> rows(p->h_ilor.begin() + (size_t)l0 * p->niso,
                              p->h_ilor.begin() + (size_t)l1 * p->niso);
        std::sort(rows.begin(), rows.end());
        rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        rc = pb_voigt_ensure_rows(sub->voigt, rows.data(), (int)rows.size(), s);
        if (rc)
            return rc;
        l0 = l1;
    }
    if (nlayers > p->pred_cap) {
        PB_HIP(hipStreamSynchronize(s));
        (void)hipFree(p->d_pred_f);
        (void)hipFree(p->d_ok);
        (void)hipFree((void *)p->d_pred_mask);
        p->d_pred_f = p->d_ok = nullptr;
        p->d_pred_mask = nullptr;
        p->pred_cap = 0;
        PB_HIP(hipMalloc(&p->d_pred_f, (size_t)nlayers * 4));
        PB_HIP(hipMalloc(&p->d_ok, (size_t)nlayers * 4));
        PB_HIP(hipMalloc((void **)&p->d_pred_mask, (size_t)nlayers * sizeof(void *)));
        p->pred_cap = nlayers;
        p->pred_dirty = true;
    }
    if (p->pred_dirty) {
        PB_REQUIRE(capturing == hipStreamCaptureStatusNone,
                   "pb_lbl_extinction: the run plan of a `resolution` call changed while a graph "
                   "was being captured");
        std::vector<const uint8_t *> masks((size_t)nlayers);
        for (int layer = 0; layer < nlayers; layer++) {
            pb_lbl::DynSub *sub = nullptr;
            const int rc = dyn_subplan(p, p->h_ofactor[(size_t)layer], s, &sub);
            if (rc)
                return rc;
            masks[(size_t)layer] = sub->voigt->d_rowmask;
        }
        PB_HIP(hipMemcpyAsync(p->d_pred_f, p->h_ofactor.data(), (size_t)nlayers * 4,
                              hipMemcpyHostToDevice, s));
        PB_HIP(hipMemcpyAsync((void *)p->d_pred_mask, masks.data(), (size_t)nlayers * sizeof(void *),
                              hipMemcpyHostToDevice, s));
        PB_HIP(hipStreamSynchronize(s));                  // (`masks` is a local; rare)
        p->pred_dirty = false;
    }
    k_dyn_check<<<pb::div_up(nlayers, 64), 64, 0, s>>>(p->d_ok, p->ls_ofactor, p->li_ilor,
                                                      p->d_pred_f, p->d_pred_mask, nlayers, p->niso);
    PB_LAUNCH_CHECK();
    const int lanes = tn.dyn_streams;
    if (lanes > 1 && p->dyn_streams.empty()) {
        PB_HIP(hipEventCreateWithFlags(&p->dyn_fork, hipEventDisableTiming));
        for (int k = 0; k < 8; k++) {
            hipStream_t t;
            hipEvent_t e;
            PB_HIP(hipStreamCreateWithFlags(&t, hipStreamNonBlocking));
            p->dyn_streams.push_back(t);
            PB_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            p->dyn_join.push_back(e);
        }
    }
    const bool timed = p->ev_used + 2 <= (int)p->ev.size();
    if (timed)
        PB_HIP(hipEventRecord(p->ev[p->ev_used], s));
    if (lanes > 1) {
        PB_HIP(hipEventRecord(p->dyn_fork, s));        // ext as the caller left it (zeroed, or sums so far)
        for (int k = 0; k < lanes; k++)
            PB_HIP(hipStreamWaitEvent(p->dyn_streams[(size_t)k], p->dyn_fork, 0));
    }
    p->last_gather = 6;
    p->dyn_runs = 0;
    p->dyn_call++;
    const double w_lo = p->h_wn[(size_t)wbegin], w_hi = p->h_wn[(size_t)(wbegin + wcount - 1)];
    int rc = PB_OK;
    // Dynamic sampling keeps the samples per line and layer about constant, so a run costs about
    // its layers (c2-res: 43 us per layer in runs of 14-18, 55-200 us for a run of one) plus its
    // small launches.  Runs that fill the chip by themselves queue on side stream 0; the others
    // (deep layers: one or two layers on a short grid) are dealt to the remaining side streams,
    // least work first, and run in the shadow of the large ones.
    double load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int nbig = tn.dyn_big;
    for (int l0 = 0; l0 < nlayers && rc == PB_OK;) {
        const int f = p->h_ofactor[(size_t)l0];
        // (a run's dynamic-grid sums stay below 1 GiB: fine factors on long fine grids)
        const int64_t run_max = std::max<int64_t>(
            1, ((int64_t)1 << 27) / ((int64_t)a.nrows * (1 + (l->onwn - 1) / f)));
        int l1 = l0 + 1;
        while (l1 < nlayers && l1 - l0 < run_max && p->h_ofactor[(size_t)l1] == f)
            l1++;
        pb_lbl::DynSub *sub = nullptr;
        rc = dyn_subplan(p, f, s, &sub);
        if (rc)
            break;
        // a factor that comes back later in the same call (a temperature inversion) shares the
        // sub-plan's workspaces with its first run: same side stream, hence in order
        int lane = 0;
        const int64_t groups = (int64_t)(l1 - l0) * pb::div_up((int64_t)sub->plan->nwave, (int64_t)4096);
        const int lo = groups < 512 ? std::min(nbig, lanes - 1) : 0;
        const int hi = groups < 512 ? lanes : std::min(nbig, lanes);
        lane = lo;
        for (int k = lo + 1; k < hi; k++)
            if (load[k] < load[lane])
                lane = k;
        if (sub->call == p->dyn_call)
            lane = sub->lane;
        load[lane] += 60.0 + 45.0 * (l1 - l0);
        sub->call = p->dyn_call;
        sub->lane = lane;
        hipStream_t t = lanes > 1 ? p->dyn_streams[(size_t)lane] : s;
        pb_lbl *q = sub->plan;
        {
            // the Lorentz rows of the re-cut table that the layers of this run read
            std::vector<int> rows(p->h_ilor.begin() + (size_t)l0 * p->niso,
                                  p->h_ilor.begin() + (size_t)l1 * p->niso);
            std::sort(rows.begin(), rows.end());
            rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
            rc = pb_voigt_ensure_rows(sub->voigt, rows.data(), (int)rows.size(), t);
            if (rc)
                break;
        }
        q->ethresh = p->ethresh;
        q->concurrency = std::max(p->concurrency, 1);
        if (q->isoiext != p->isoiext) {
            rc = pb_lbl_set_isoiext(q, p->isoiext.data());
            if (rc)
                break;
        }
        // the dynamic samples the outputs of this call read (one of margin on either side)
        const double step = l->ownstep * f;
        const int64_t dn = q->nwave;
        int64_t d0 = (int64_t)((w_lo - p->wn0) / step) - 1;
        int64_t d1 = (int64_t)((w_hi - p->wn0) / step) + 3;
        d0 = std::max<int64_t>(0, std::min(d0, dn - 1));
        d1 = std::max(d0 + 1, std::min(d1, dn));
        const int nl = l1 - l0;
        const size_t need = (size_t)nl * a.nrows * (size_t)(d1 - d0) * 8;
        if (need > sub->ktmp_bytes) {
            if (hipStreamSynchronize(t) != hipSuccess) {
                // (not PB_HIP: the side streams below must be joined on every path)
                pb::set_error("pb_lbl_extinction: side stream failed: %s",
                              hipGetErrorString(hipGetLastError()));
                rc = PB_ERR_HIP;
                break;
            }
            (void)hipFree(sub->ktmp);
            sub->ktmp = nullptr;
            sub->ktmp_bytes = 0;
            if (hipMalloc(&sub->ktmp, need) != hipSuccess) {
                pb::set_error("pb_lbl_extinction: cannot allocate %zu B of dynamic-grid sums", need);
                rc = PB_ERR_NOMEM;
                break;
            }
            sub->ktmp_bytes = need;
        }
        const Call run{sub->ktmp, d0, d1 - d0, c.temp + l0, c.dens + (int64_t)l0 * p->nmol,
                       c.isoz + (int64_t)l0 * c.zs1, c.zs0, c.zs1, nl, c.add, false};
        rc = lbl_extinction(q, run, t, 0);
        if (rc)
            break;
        // (pb_lbl_last_state / pb_lbl_kmax_buffer of this plan report the run's maxima)
        k_dyn_kmax<<<pb::div_up(nl * a.nrows, 64), 64, 0, t>>>(
            p->kmax_bits + (size_t)l0 * a.nrows, q->kmax_bits, p->d_ok + l0, nl, a.nrows);
        if (hipGetLastError() != hipSuccess) {
            pb::set_error("pb_lbl_extinction: copy of the per-row maxima failed");
            rc = PB_ERR_HIP;
            break;
        }
        dim3 grid((unsigned)pb::div_up(wcount, (int64_t)kBlock), (unsigned)(nl * a.nrows));
        k_dyn_interp<<<grid, kBlock, 0, t>>>(c.ext + (int64_t)l0 * a.nrows * wcount, sub->ktmp,
                                            p->d_wn, p->wn0, p->ls_dwnstep + l0, d0, d1 - d0,
                                            wbegin, wcount, a.nrows, p->d_ok + l0);
        if (hipGetLastError() != hipSuccess) {
            pb::set_error("pb_lbl_extinction: k_dyn_interp launch failed");
            rc = PB_ERR_HIP;
            break;
        }
        p->dyn_runs++;
        l0 = l1;
    }
    // (joined on every path: the caller's stream must not run ahead of a side stream)
    // Best effort, lane by lane: a failing record / wait must not leave the other lanes unjoined
    // (their kernels still write ext_d and the sub-plans' sums); a lane that cannot be joined
    // through its event is waited for on the host.
    if (lanes > 1)
        for (int k = 0; k < lanes; k++) {
            hipStream_t t = p->dyn_streams[(size_t)k];
            if (hipEventRecord(p->dyn_join[(size_t)k], t) != hipSuccess ||
                hipStreamWaitEvent(s, p->dyn_join[(size_t)k], 0) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(t);
                if (rc == PB_OK) {
                    pb::set_error("pb_lbl_extinction: joining side stream %d failed", k);
                    rc = PB_ERR_HIP;
                }
            }
        }
    if (rc)
        return rc;
    if (timed) {
        PB_HIP(hipEventRecord(p->ev[p->ev_used + 1], s));
        p->ev_used += 2;
    }
    return PB_OK;
}

}  // namespace pbx

#ifdef PB_EXPERIMENTS
extern "C" {

int pb_lbl_set_dyn_predict(pb_lbl *p, int on)
{
    PB_REQUIRE(p, "pb_lbl_set_dyn_predict: null handle");
    PB_REQUIRE(p->resolution, "pb_lbl_set_dyn_predict: the plan is not a `resolution` plan");
    p->dyn_predict = on ? 1 : 0;
    return PB_OK;
}

int pb_lbl_dyn_stats(pb_lbl *p, int64_t stats[3])
{
    PB_REQUIRE(p && stats, "pb_lbl_dyn_stats: null pointer");
    stats[0] = p->dyn_spec_calls;
    stats[1] = p->dyn_sync_calls;
    stats[2] = p->dyn_mispredicted;
    return PB_OK;
}

}  // extern "C"
#endif  // PB_EXPERIMENTS
