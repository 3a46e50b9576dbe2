// The cloudy column walk of the walker-batched retrieval path, stated once for the flux kernels
// (pb_clouds.hip) and the band contribution kernels (pb_contribution.hip): what a walker's cloudy
// column is (ec + ec_cloud down to its deck), how the patchy fraction mixes it with the clear one,
// and the transit walk over blocks of impact parameters with the ray-path segments staged in LDS.
// Everything is __forceinline__ and templated on what the kernels are templated on; what a kernel
// does with a block's optical depths stays in the kernel.
#pragma once

#include "pb_common.h"

namespace pb {

// ec_cloud = sum_m cs_m[sample] f_m[walker, layer] at this thread's sample (pb_cloud_terms): the
// cross sections in registers (a gray model: 1), the factors wave-uniform scalar loads, the
// models' terms added in their order
struct CloudWalk {
    double cs[PB_CLOUD_MAX];
    const double *f;            // this walker's factors [L][nr]
    int nr;

    __device__ __forceinline__ void init(const pb_cloud_terms &cl, int w, int64_t col, int nlayers)
    {
        nr = cl.nr;
        f = cl.f_d + (int64_t)w * nlayers * cl.nr;
#pragma unroll
        for (int m = 0; m < PB_CLOUD_MAX; m++) {
            cs[m] = 0.0;
            if (m < cl.nr)
                cs[m] = cl.cs_d[m] ? cl.cs_d[m][(int64_t)w * cl.cs_stride[m] + col] : 1.0;
        }
    }
    __device__ __forceinline__ double at(int layer) const
    {
        const cdbl_t fl = (cdbl_t)(unsigned long long)(f + (int64_t)layer * nr);
        double sum = 0.0;
#pragma unroll
        for (int m = 0; m < PB_CLOUD_MAX; m++)
            if (m < nr)
                sum += cs[m] * fl[m];
        return sum;
    }
};

// the walker's deck layer, inside the grid whatever deck_itop holds (wave-uniform)
__device__ __forceinline__ int deck_layer(const int32_t *deck_itop, int w, int nlayers)
{
    return min(max(uniform_i32(deck_itop + w), 0), nlayers - 1);
}

// the walker's cloudy fraction, clamped to [0, 1] (NaN stays NaN), and the mix of the two columns
// (pyrat/spectrum.py:362, 384)
__device__ __forceinline__ double patchy_fraction(const double *f_patchy, int w)
{
    const double f = uniform_f64(f_patchy + w);
    return f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
}
__device__ __forceinline__ double patchy_mix(double f, double cloudy, double clear)
{
    return f * cloudy + (1.0 - f) * clear;
}

// Infinite opacity: the fma over the rows of a block (depth_block) is predicate-free, and the
// staged zeros of the rows ABOVE a layer would meet an infinite sum of that layer as
// 0 * inf = NaN, where the reference never touches the layer for those rows.  The sum of a
// segment's two layers is therefore capped at the largest finite double: 0 * it = 0 for the rows
// above, and the rows that do include the layer still get an optical depth beyond any maxdepth
// whose exp(-depth) is 0, as with +inf.  Every finite sum keeps its bits; NaN stays NaN.
__device__ __forceinline__ double finite_sum(double s)
{
    return s > 0x1.fffffffffffffp+1023 ? 0x1.fffffffffffffp+1023 : s;
}

// The ray-path segments of the impact parameters rb .. rb + kRows - 1 of a walker's packed
// triangle, staged by the workgroup's kBlock threads: s_path[segment][row], rlast segments, zero
// where segment >= row or row > rlast.  Element e = segment * kRows + row goes to thread
// e % kBlock, so a thread keeps one row.  No barrier: the caller places it.
template <int kRows, int kBlock>
__device__ __forceinline__ void stage_path_block(double *s_path, const double *path, int rb,
                                                 int rlast)
{
    static_assert(kBlock % kRows == 0, "a thread stages the segments of one row");
    const int k = threadIdx.x % kRows, r = rb + k;
    for (int i = threadIdx.x / kRows; i < rlast; i += kBlock / kRows)
        s_path[i * kRows + k] = (r <= rlast && i < r) ? path[((int64_t)r * (r - 1)) / 2 + i] : 0.0;
}

// The optical depths of a block's rows at this thread's column: tau[k] = sum over the segments
// i < nseg of s_path[i][k] (ec[itop + i] + ec[itop + i + 1]), src = the column at layer itop with
// stride nwave (optic_depth.py:103-112).  kTwo: tau_c the same on ec + ec_cloud, else untouched.
template <int kRows, bool kTwo>
__device__ __forceinline__ void depth_block(double (&tau)[kRows], double (&tau_c)[kTwo ? kRows : 1],
                                            const double *src, int nwave, int nseg,
                                            const double *s_path, const CloudWalk &cloud, int itop)
{
#pragma unroll
    for (int k = 0; k < kRows; k++)
        tau[k] = 0.0;
#pragma unroll
    for (int k = 0; k < (kTwo ? kRows : 1); k++)
        tau_c[k] = 0.0;
    if (nseg <= 0)
        return;
    double prev = src[0];
    double prev_c = kTwo ? prev + cloud.at(itop) : 0.0;
#pragma unroll 2
    for (int i = 0; i < nseg; i++) {
        const double next = src[(int64_t)(i + 1) * nwave];
        const double s = finite_sum(next + prev);
        prev = next;
        const double *pk = s_path + i * kRows;      // LDS broadcast reads
        if constexpr (kTwo) {
            const double next_c = next + cloud.at(itop + i + 1);
            const double s_c = finite_sum(next_c + prev_c);
            prev_c = next_c;
#pragma unroll
            for (int k = 0; k < kRows; k++) {
                tau[k] = fma(pk[k], s, tau[k]);
                tau_c[k] = fma(pk[k], s_c, tau_c[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kRows; k++)
                tau[k] = fma(pk[k], s, tau[k]);
        }
    }
}

// a pb_cloud_terms of an entry point (null: no cloud-type opacity)
inline int check_cloud(const pb_cloud_terms *cloud, const char *who)
{
    if (!cloud)
        return PB_OK;
    PB_REQUIRE(cloud->nr >= 0 && cloud->nr <= PB_CLOUD_MAX, "%s: 0 ... %d cloud terms (got %d)",
               who, PB_CLOUD_MAX, cloud->nr);
    PB_REQUIRE(cloud->nr == 0 || cloud->f_d, "%s: null cloud factors", who);
    for (int m = 0; m < cloud->nr; m++)
        PB_REQUIRE(cloud->cs_stride[m] >= 0, "%s: negative cross-section stride", who);
    return PB_OK;
}

}  // namespace pb
