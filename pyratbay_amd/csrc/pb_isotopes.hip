// Walker-batched retrieval path: the isotope ratios of the table's slots (Line_Sample's
// isotope_ratios, pyratbay/opacity/line_sampling.py:282-298, 451-456).  One launch scales every
// walker's densities by the ratios of its own parameters, before the table is interpolated.
#include <cfloat>

#include "pb_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kElementsPerLane = 4;
constexpr int kMaxSpec = 4096;                // the ratios of a walker in LDS: 32 KiB

// Grid (walker, block of the walker's slab dens[L][nspec]).  Every workgroup forms its walker's
// ratios once: the first nlabelled lanes take the constants and 10**par of the labelled slots
// into LDS, then the fill slots' lanes form 1 - (r_a + r_b + ...), summed left to right, every
// operation rounded on its own; unlabelled slots are 1.0.  Then consecutive lanes take
// consecutive elements of the slab: dens_out = dens_in * ratio, one multiply.  A walker with a
// ratio that is not finite or negative gets zeros in dens_out and temps_out and PB_ISO_REJECT.
__global__ __launch_bounds__(kBlock) void k_iso_density(
    double *dens_out, double *temps_out, double *ratios_out, int32_t *reject_out,
    const double *dens_in, const double *temps_in, const double *pars, const pb_iso_model m,
    int nlayers)
{
    extern __shared__ double s_ratio[];                   // [nspec]
    __shared__ double s_lab[PB_ISO_MAX_SLOTS];
    const int t = threadIdx.x;
    const int64_t w = blockIdx.x;
    const int nspec = m.nspec;
    for (int s = t; s < nspec; s += kBlock)
        s_ratio[s] = 1.0;
    const bool labelled = t < m.nlabelled;
    if (labelled && m.kind[t] != PB_ISO_FILL)
        s_lab[t] = m.kind[t] == PB_ISO_FREE ? pow(10.0, pars[w * m.npars + m.par[t]])
                                            : m.constant[t];
    __syncthreads();
    int bad = 0;
    if (labelled) {
        double r;
        if (m.kind[t] == PB_ISO_FILL) {
            double sum = s_lab[m.fill[t][0]];
            for (int k = 1; k < m.nfill[t]; k++)
                sum += s_lab[m.fill[t][k]];
            r = 1.0 - sum;
        } else {
            r = s_lab[t];
        }
        s_ratio[m.slot[t]] = r;
        bad = !(r >= 0.0 && r <= DBL_MAX);               // negative, infinite or NaN
    }
    const int reject = __syncthreads_or(bad);

    if (blockIdx.y == 0) {
        if (ratios_out)
            for (int s = t; s < nspec; s += kBlock)
                ratios_out[w * nspec + s] = s_ratio[s];
        if (t == 0)
            reject_out[w] = reject ? PB_ISO_REJECT : 0;
        for (int l = t; l < nlayers; l += kBlock)
            temps_out[w * nlayers + l] = reject ? 0.0 : temps_in[w * nlayers + l];
    }
    // (at most INT32_MAX elements in the slab, a grid stride below 2^24: 32-bit indices)
    const uint32_t n = (uint32_t)nlayers * (uint32_t)nspec;
    const int64_t base = w * (int64_t)n;
    for (uint32_t e = blockIdx.y * kBlock + t; e < n; e += gridDim.y * kBlock)
        dens_out[base + e] = reject ? 0.0 : dens_in[base + e] * s_ratio[e % (uint32_t)nspec];
}

}  // namespace

extern "C" {

int pb_iso_density(double *dens_out_d, double *temps_out_d, double *ratios_out_d,
                   int32_t *reject_out_d, const double *dens_in_d, const double *temps_in_d,
                   const double *pars_d, const pb_iso_model *model, int nlayers, int nwalkers,
                   void *stream)
{
    PB_REQUIRE(model, "pb_iso_density: null model");
    PB_REQUIRE(nlayers >= 1 && nwalkers >= 0, "pb_iso_density: bad shape");
    PB_REQUIRE(model->nspec >= 1 && model->nspec <= kMaxSpec,
               "pb_iso_density: %d table slots: 1 ... %d", model->nspec, kMaxSpec);
    PB_REQUIRE(model->nlabelled >= 0 && model->nlabelled <= PB_ISO_MAX_SLOTS &&
                   model->nlabelled <= model->nspec,
               "pb_iso_density: %d labelled slots: at most %d, and at most the %d of the table",
               model->nlabelled, PB_ISO_MAX_SLOTS, model->nspec);
    PB_REQUIRE(model->npars >= 0, "pb_iso_density: bad parameter count");
    for (int i = 0; i < model->nlabelled; i++) {
        PB_REQUIRE(model->slot[i] >= 0 && model->slot[i] < model->nspec,
                   "pb_iso_density: labelled slot %d is table slot %d of %d", i, model->slot[i],
                   model->nspec);
        for (int j = 0; j < i; j++)
            PB_REQUIRE(model->slot[j] != model->slot[i],
                       "pb_iso_density: table slot %d is labelled twice", model->slot[i]);
        const int kind = model->kind[i];
        PB_REQUIRE(kind == PB_ISO_CONST || kind == PB_ISO_FREE || kind == PB_ISO_FILL,
                   "pb_iso_density: labelled slot %d: kind %d", i, kind);
        if (kind == PB_ISO_FREE) {
            PB_REQUIRE(model->par[i] >= 0 && model->par[i] < model->npars,
                       "pb_iso_density: labelled slot %d reads column %d of %d", i,
                       model->par[i], model->npars);
            PB_REQUIRE(pars_d || nwalkers == 0,
                       "pb_iso_density: a free slot needs pars (null: constants only)");
        }
        if (kind == PB_ISO_FILL) {
            PB_REQUIRE(model->nfill[i] >= 1 && model->nfill[i] <= PB_ISO_MAX_FILLERS,
                       "pb_iso_density: labelled slot %d has %d fillers: 1 ... %d", i,
                       model->nfill[i], PB_ISO_MAX_FILLERS);
            for (int k = 0; k < model->nfill[i]; k++) {
                const int f = model->fill[i][k];
                PB_REQUIRE(f >= 0 && f < model->nlabelled && model->kind[f] != PB_ISO_FILL,
                           "pb_iso_density: labelled slot %d: filler %d is no labelled slot, or "
                           "a fill slot itself", i, f);
            }
        }
    }
    PB_REQUIRE((int64_t)nlayers * model->nspec <= INT32_MAX,
               "pb_iso_density: a walker's slab of %d x %d elements is too large", nlayers,
               model->nspec);
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(dens_out_d && temps_out_d && reject_out_d && dens_in_d && temps_in_d,
               "pb_iso_density: null pointer");
    const int64_t n = (int64_t)nlayers * model->nspec;
    const int blocks = (int)std::min<int64_t>(pb::div_up(n, kBlock * kElementsPerLane), 65535);
    k_iso_density<<<dim3(nwalkers, blocks), kBlock, model->nspec * sizeof(double),
                    pb::as_stream(stream)>>>(dens_out_d, temps_out_d, ratios_out_d, reject_out_d,
                                             dens_in_d, temps_in_d, pars_d, *model, nlayers);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
