// Radiative equilibrium on the device (Pyrat.radiative_equilibrium, pyrat/pyrat_obj.py:559-646 ->
// spectrum/radiative_transfer.py:141-270) for a batch of profiles at fixed volume mixing ratios,
// without convection.  One iteration is three launches and no host work: the interpolation of the
// table (pb_interp_ec_batch[_cont]), k_two_stream_net_batch and k_radeq_update.
//
// k_two_stream_net_batch is k_two_stream_batch (pb_two_stream.hip: the same statements of
// pb_two_stream.h in the same order, ec consumed, trans in the work buffer, the profile's
// temperatures and intervals in LDS; flux_up[0] has the same bits) that ALSO forms, at every layer
// of both sweeps, the trapezoid contribution t_j flux[i][j] of its column to the bolometric fluxes
// Qdown[i], Qup[i] (radiative_transfer.py:208-209) and reduces it over the 64 columns of its
// wavefront; the four wavefronts of a workgroup leave their sums in LDS and are added in order
// behind the one barrier at the end of the kernel.  A part is a workgroup of 256 columns:
// parts[nw][npart][2][L] (0: up, 1: down), npart = ceil(W / 256).  No atomics: the xor butterfly
// gives every lane the same sum (IEEE addition commutes), lane 0 stores it, and k_radeq_update adds
// the parts in a fixed order (part_groups below) -- two runs give the same bits.
//
// k_radeq_update: one workgroup per profile, the reference's statements of
// radiative_transfer.py:207-237 in their order on profile-length vectors in LDS, then the
// atmosphere of the next iteration (ideal-gas densities and the hydrostatic radius of
// pb_atm_profile.h) in the same launch.  Its state -- dt_scale, the last four rows of sign(dF), the
// iteration counter -- lives on the device.
#include "pb_atm_profile.h"
#include "pb_common.h"
#include "pb_planck.h"
#include "pb_two_stream.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kUpdate = 256;
constexpr int kMaxRadius = 8;                        // int(4 * 2.0 + 0.5): sigma is clipped to 2
constexpr int kRows = 6;                             // profile-length vectors of the update in LDS
constexpr int kStage = 2 * kUpdate;                  // doubles of LDS for the groups' partial sums

// The order the parts are added in: up to kUpdate / L groups of consecutive parts (one thread per
// (group, layer); a single group above kUpdate layers), each added left to right from 0, then the
// groups left to right from 0.
__host__ __device__ inline int part_groups(int nlayers, int nparts)
{
    if (nlayers > kUpdate)
        return 1;
    const int g = kUpdate / nlayers < nparts ? kUpdate / nlayers : nparts;
    return g > 1 ? g : 1;
}
constexpr double kSigmaSB = 5.6703744191844314e-08 * 1e3;   // pc.sigma = sc.sigma * 1e3

using pb::planck_factor;
using pb::planck_q;
using pb::planck_terms;
using pb::two_stream_down;
using pb::two_stream_trans;
using pb::two_stream_up;

// the sum over the wavefront, the same bits in every lane
__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = kWave / 2; off > 0; off >>= 1)
        v += __shfl_xor(v, off, kWave);
    return v;
}

// grid (blocks of 256 columns, walkers) as k_two_stream_batch.  Lanes past nwave of the last live
// wavefront take part in the sums with 0 and touch no global memory; a wavefront wholly past nwave
// leaves zeros in its LDS rows.  LDS: the 3 L doubles of k_two_stream_batch, then
// s_q[wavefront][2][L].
__global__ __launch_bounds__(kBlock) void k_two_stream_net_batch(
    double *__restrict__ flux, double *__restrict__ parts, double *__restrict__ ec,
    const double *__restrict__ intervals, const double *__restrict__ wn,
    const double *__restrict__ tw, const double *__restrict__ temp,
    const double *__restrict__ f_int, int f_int_stride, const double *__restrict__ flux_top,
    int flux_top_stride, double *__restrict__ work, int nlayers, int nwave, int npart)
{
    extern __shared__ double s_kt[];
    double *s_h = s_kt + 2 * nlayers;
    double *s_q = s_kt + 3 * nlayers;
    const int wk = blockIdx.y;
    for (int k = threadIdx.x; k < nlayers - 1; k += kBlock)
        s_h[k] = intervals[(int64_t)wk * (nlayers - 1) + k];
    planck_terms(s_kt, temp + (int64_t)wk * nlayers, nlayers);        // (ends with the barrier)
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const bool live = j < nwave;
    const bool writer = (threadIdx.x & (kWave - 1)) == 0;
    double *q_up = s_q + (threadIdx.x >> 6) * 2 * nlayers;
    double *q_down = q_up + nlayers;
    if (blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1)) >= nwave) {
        // (the whole wavefront: nothing to add)
        for (int i = threadIdx.x & (kWave - 1); i < 2 * nlayers; i += kWave)
            q_up[i] = 0.0;
    } else {
        double w = 0.0, factor = 0.0, tj = 0.0, down = 0.0, prev = 0.0, cur = 0.0, bprev = 0.0;
        if (live) {
            ec += (int64_t)wk * nlayers * nwave + j;
            work += (int64_t)wk * (nlayers - 1) * nwave + j;
            w = wn[j];
            tj = tw[j];
            factor = planck_factor(w);
            // downward sweep from the irradiation at the top (itop = 0: spectrum.py:498-509)
            down = flux_top ? flux_top[(int64_t)wk * flux_top_stride + j] : 0.0;
            prev = ec[0];
            cur = nlayers > 1 ? ec[nwave] : 0.0;
            bprev = planck_q(factor, w, s_kt[0], s_kt[nlayers]);
        }
        double depth = 0.0;
        for (int i = 0; i < nlayers - 1; i++) {
            const double qd = wave_sum(tj * down);                         // flux_down[i]
            if (writer)
                q_down[i] = qd;
            if (live) {
                const double ahead = ec[(int64_t)min(i + 2, nlayers - 1) * nwave];
                const double dnext = depth + 0.5 * s_h[i] * (cur + prev);
                const double dtau0 = dnext - depth;
                const double trans = two_stream_trans(dtau0);
                const double bnext = planck_q(factor, w, s_kt[i + 1], s_kt[nlayers + i + 1]);
                down = two_stream_down(down, trans, dtau0, bprev, bnext);
                ec[(int64_t)i * nwave] = dtau0;
                work[(int64_t)i * nwave] = trans;
                depth = dnext;
                prev = cur;
                cur = ahead;
                bprev = bnext;
            }
        }
        {
            const double qd = wave_sum(tj * down);
            if (writer)
                q_down[nlayers - 1] = qd;
        }
        double up = 0.0;
        if (live)
            up = down + (f_int ? f_int[(int64_t)wk * f_int_stride + j] : 0.0);
        {
            const double qu = wave_sum(tj * up);                           // flux_up[L-1]
            if (writer)
                q_up[nlayers - 1] = qu;
        }
        // upward sweep; bprev = B[L-1]
        double dtau0 = 0.0, trans = 0.0;
        if (live && nlayers > 1) {
            dtau0 = ec[(int64_t)(nlayers - 2) * nwave];
            trans = work[(int64_t)(nlayers - 2) * nwave];
        }
        for (int i = nlayers - 2; i >= 0; i--) {
            if (live) {
                const int inext = max(i - 1, 0);
                const double dtau_next = ec[(int64_t)inext * nwave];
                const double trans_next = work[(int64_t)inext * nwave];
                const double blo = planck_q(factor, w, s_kt[i], s_kt[nlayers + i]);
                up = two_stream_up(up, trans, dtau0, blo, bprev);
                bprev = blo;
                dtau0 = dtau_next;
                trans = trans_next;
            }
            const double qu = wave_sum(tj * up);                           // flux_up[i]
            if (writer)
                q_up[i] = qu;
        }
        if (live)
            flux[(int64_t)wk * nwave + j] = up;
    }
    // the workgroup's part: its wavefronts in order
    __syncthreads();
    double *part = parts + ((int64_t)wk * npart + blockIdx.x) * 2 * nlayers;
    for (int i = threadIdx.x; i < 2 * nlayers; i += kBlock) {
        double v = s_q[i];
        for (int wv = 1; wv < kBlock / kWave; wv++)
            v += s_q[wv * 2 * nlayers + i];
        part[i] = v;
    }
}

// ---------------------------------------------------------------------------------- the update

// np.add.reduce of n contiguous doubles (NumPy's pairwise sum: sequential below 8 elements, 8
// running sums combined as a tree up to 128, halves rounded down to a multiple of 8 above)
__device__ double np_sum_block(const double *a, int n)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; i++)
            res += a[i];
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; j++)
        r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++)
            r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++)
        res += a[i];
    return res;
}
template <int kDepth>
__device__ double np_sum(const double *a, int n)
{
    if (n <= 128)
        return np_sum_block(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_sum<kDepth - 1>(a, n2) + np_sum<kDepth - 1>(a + n2, n - n2);
}
template <>
__device__ double np_sum<0>(const double *a, int n)
{
    // (four halvings leave at most 1024 / 16 + 7 = 71 elements of PB_ATM_MAX_LAYERS = 1024: halves
    // are rounded down to a multiple of 8, so three leave up to 135, e.g. at 1023)
    return np_sum_block(a, n);
}

// scipy.ndimage's _gaussian_kernel1d(sigma, 0, radius) with radius = int(4 sigma + 0.5) into
// w[0 .. 2 radius]; returns the radius.  ONE thread.
__device__ int gauss_weights(double sigma, double *w)
{
    // (a NaN sigma -- a NaN flux -- gives NaN weights of radius 0, never an index past the row)
    const int radius = sigma == sigma ? min(max((int)(4.0 * sigma + 0.5), 0), kMaxRadius) : 0;
    const double c = -0.5 / (sigma * sigma);
    for (int x = -radius; x <= radius; x++)
        w[x + radius] = exp(c * (double)(x * x));
    const double sum = np_sum_block(w, 2 * radius + 1);
    for (int x = 0; x <= 2 * radius; x++)
        w[x] = w[x] / sum;
    return radius;
}

// index i of the line extended by mode 'reflect' (d c b a | a b c d | d c b a, repeated)
__device__ __forceinline__ int reflect(int i, int n)
{
    int m = i % (2 * n);
    if (m < 0)
        m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// scipy.ndimage.correlate1d with symmetric weights at element l: the centre tap, then the pairs
// from the outermost inwards
__device__ double correlate_reflect(const double *s, int l, int n, const double *w, int radius)
{
    double acc = s[l] * w[radius];
    for (int k = -radius; k < 0; k++)
        acc += (s[reflect(l + k, n)] + s[reflect(l - k, n)]) * w[k + radius];
    return acc;
}

__device__ __forceinline__ double np_sign(double x)
{
    return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x));
}

__global__ __launch_bounds__(kUpdate) void k_radeq_update(pb_radeq a, int init_only)
{
    extern __shared__ double s_row[];
    const int L = a.nlayers;
    const int tid = threadIdx.x;
    const int64_t w = blockIdx.x;
    double *s_t = s_row;              // T of this iteration
    double *s_q = s_t + L;            // Q_net; |dT|; the hydrostatic integrand
    double *s_df = s_q + L;           // dF; the cumulative hydrostatic integral
    double *s_a = s_df + L;           // dt_scale_tmp before its filter; T of the next iteration
    double *s_b = s_a + L;            // dt_scale_tmp; the radius
    double *s_tn = s_b + L;           // T + dT
    double *s_w = s_tn + L;           // [2 kMaxRadius + 1] filter weights
    // the groups' partial sums [groups][2][L]: groups * L <= kUpdate up to kUpdate layers, i.e. at
    // most kStage doubles behind the weights; above that ONE group, 2 L doubles, which lie over
    // s_a and s_b (both dead until the sums have been read, a barrier before their first store)
    double *s_part = L > kUpdate ? s_a : s_w + 2 * kMaxRadius + 1;
    __shared__ int s_radius;
    const int k = a.iter_d[w];
    // (a launch beyond the rows of the history does nothing)
    if (!init_only && (k < 0 || k + 1 >= a.nrows))
        return;
    for (int l = tid; l < L; l += kUpdate)
        s_t[l] = a.temp_d[w * L + l];
    double *s_next = s_t;
    if (!init_only) {
        // Qup, Qdown: the parts in the order of part_groups; Q_net
        const int groups = part_groups(L, a.nparts);
        const int chunk = (a.nparts + groups - 1) / groups;
        for (int idx = tid; idx < groups * L; idx += kUpdate) {
            const int g = idx / L, l = idx - g * L;
            double qu = 0.0, qd = 0.0;
            for (int p = g * chunk; p < min((g + 1) * chunk, a.nparts); p++) {
                const double *q = a.parts_d + ((w * a.nparts + p) * 2) * L;
                qu += q[l];
                qd += q[L + l];
            }
            s_part[(2 * g) * L + l] = qu;
            s_part[(2 * g + 1) * L + l] = qd;
        }
        __syncthreads();
        for (int l = tid; l < L; l += kUpdate) {
            double qu = 0.0, qd = 0.0;
            for (int g = 0; g < groups; g++) {
                qu += s_part[(2 * g) * L + l];
                qd += s_part[(2 * g + 1) * L + l];
            }
            a.q_up_d[w * L + l] = qu;
            a.q_down_d[w * L + l] = qd;
            s_q[l] = qu - qd;
        }
        if (tid == 0)
            gauss_weights(1.5, s_w);
        __syncthreads();
        // dF, its sign, the wobbling layers, dt_scale_tmp before the filter
        const int nprev = min(k, 4);
        for (int l = tid; l < L; l += kUpdate) {
            const double dF = l == 0 ? 0.0 : s_q[l] - s_q[l - 1];
            const double sg = np_sign(dF);
            bool wobble = false;
            for (int r = 1; r <= nprev; r++)
                if ((a.signs_d[(w * 4 + ((k - r) & 3)) * L + l] - sg) != 0.0)
                    wobble = true;
            a.signs_d[(w * 4 + (k & 3)) * L + l] = sg;
            if (a.wobble_d)
                a.wobble_d[w * L + l] = wobble;
            double v = a.dt_scale_d[w * L + l] * (wobble ? 0.5 : 1.15);
            v = v < 1.0 ? 1.0 : v;                   // np.clip = minimum(maximum(x, lo), hi)
            v = v > 1.0e8 ? 1.0e8 : v;
            s_df[l] = dF;
            s_a[l] = v;
        }
        __syncthreads();
        for (int l = tid; l < L; l += kUpdate) {
            const double dts = correlate_reflect(s_a, l, L, s_w, 6);
            const double dF = s_df[l], t = s_t[l];
            const double dT = ((dts * np_sign(dF)) * pow(fabs(dF), 0.1)) /
                              ((kSigmaSB * pow(t, 3.0)) * a.dpress_d[l]);
            s_b[l] = dts;
            s_tn[l] = t + dT;
            s_q[l] = fabs(dT);
        }
        __syncthreads();
        if (tid == 0) {
            s_tn[0] = s_tn[1];                       // isothermal top
            double sigma = (np_sum<4>(s_q, L) / (double)L) / 10.0;
            sigma = sigma < 0.75 ? 0.75 : sigma;
            sigma = sigma > 2.0 ? 2.0 : sigma;
            s_radius = gauss_weights(sigma, s_w);
            a.iter_d[w] = k + 1;
            if (a.sigma_d)
                a.sigma_d[w] = sigma;
        }
        __syncthreads();
        const int radius = s_radius;
        for (int l = tid; l < L; l += kUpdate) {
            double v = l < L - 1 ? correlate_reflect(s_tn, l, L, s_w, radius) : s_tn[l];
            v = v < a.tmin ? a.tmin : v;
            v = v > a.tmax ? a.tmax : v;
            s_a[l] = v;
            a.dt_scale_d[w * L + l] = s_b[l];
            a.temps_d[(w * a.nrows + k + 1) * L + l] = v;
            a.temp_d[w * L + l] = v;
        }
        __syncthreads();
        s_next = s_a;
    } else {
        __syncthreads();
    }

    // ---- the atmosphere of the next evaluation: n = vmr p / (k T) for the table's and the
    // continuum's species, consecutive threads writing consecutive elements
    const double *vmr = a.vmr_d + w * a.vmr_stride;
    for (int idx = tid; idx < L * a.ntab; idx += kUpdate) {
        const int l = idx / a.ntab, j = idx - l * a.ntab;
        a.dens_d[w * L * a.ntab + idx] = pb::atm::ideal_gas_density(
            vmr[(int64_t)l * a.nspecies + a.tab_map_d[j]], a.pressure_d[l], s_next[l]);
    }
    for (int idx = tid; idx < L * a.ncont; idx += kUpdate) {
        const int l = idx / a.ncont, j = idx - l * a.ncont;
        a.cdens_d[w * L * a.ncont + idx] = pb::atm::ideal_gas_density(
            vmr[(int64_t)l * a.nspecies + a.cont_map_d[j]], a.pressure_d[l], s_next[l]);
    }
    if (a.rmodel < 0)
        return;                                      // (a fixed radius: the caller's intervals stay)
    // ---- hydrostatic radius (atmosphere.py:397-415, 467-485) and the layer intervals
    const double *mm = a.mm_d + w * a.mm_stride;
    for (int l = tid; l < L; l += kUpdate)
        s_q[l] = pb::atm::hydro_integrand(a.rmodel, s_next[l], mm[l], a.mplanet, a.gplanet);
    __syncthreads();
    if (tid == 0)
        pb::atm::hydro_cumulative(s_df, a.lnp_d, s_q, L);
    __syncthreads();
    if (a.has_ref) {
        const double i0 = pb::atm::hydro_reference(a.pressure_d, s_df, a.p0, L);
        for (int l = tid; l < L; l += kUpdate)
            s_b[l] = pb::atm::hydro_radius(a.rmodel, s_df[l], i0, a.r0);
    } else {
        for (int l = tid; l < L; l += kUpdate)       // hydro_g without a reference: radius[-1] = 0
            s_b[l] = s_df[l] - s_df[L - 1];
    }
    __syncthreads();
    if (a.rmodel == 0 && tid == 0) {
        // hydro_m: inf above the last layer where the radius stops decreasing
        for (int l = L - 2; l >= 0; l--)
            if (s_b[l] <= s_b[l + 1]) {
                for (int i = 0; i <= l; i++)
                    s_b[i] = INFINITY;
                break;
            }
    }
    __syncthreads();
    for (int l = tid; l < L; l += kUpdate) {
        a.radius_d[w * L + l] = s_b[l];
        if (l < L - 1)
            a.intervals_d[w * (L - 1) + l] = s_b[l] - s_b[l + 1];
    }
}

}  // namespace

extern "C" {

int pb_two_stream_net_parts(int nwave)
{
    return nwave > 0 ? pb::div_up(nwave, kBlock) : 0;
}

int64_t pb_two_stream_net_work_doubles(int nlayers, int nwave, int nwalkers)
{
    if (nlayers <= 1 || nwave <= 0 || nwalkers <= 0)
        return 0;
    return (int64_t)nwalkers * (nlayers - 1) * nwave;
}

int pb_two_stream_net_batch(double *flux_d, double *parts_d, double *ec_d,
                            const double *intervals_d, const double *wn_d,
                            const double *trapz_weights_d, const double *temps_d,
                            const double *f_int_d, int f_int_stride, const double *flux_top_d,
                            int flux_top_stride, double *work_d, int nlayers, int nwave,
                            int nwalkers, void *stream)
{
    PB_REQUIRE(nlayers >= 1 && nwave >= 0 && nwalkers >= 0, "pb_two_stream_net_batch: bad shape");
    if (nwave == 0 || nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(flux_d && parts_d && ec_d && wn_d && trapz_weights_d && temps_d &&
                   (nlayers == 1 || intervals_d),
               "pb_two_stream_net_batch: null pointer");
    PB_REQUIRE((f_int_stride == 0 || f_int_stride == nwave) &&
                   (flux_top_stride == 0 || flux_top_stride == nwave),
               "pb_two_stream_net_batch: the strides of f_int and flux_top are 0 (shared) or "
               "nwave = %d (per profile), not %d and %d", nwave, f_int_stride, flux_top_stride);
    PB_REQUIRE(work_d || pb_two_stream_net_work_doubles(nlayers, nwave, nwalkers) == 0,
               "pb_two_stream_net_batch: null work (pb_two_stream_net_work_doubles doubles of "
               "device scratch)");
    const size_t lds = ((size_t)(3 + 2 * (kBlock / kWave)) * nlayers) * sizeof(double);
    PB_REQUIRE(lds <= 64 * 1024, "pb_two_stream_net_batch: %d layers: at most %d (the profile's "
               "temperatures and intervals and the workgroup's flux sums are kept in LDS)", nlayers,
               64 * 1024 / (8 * (3 + 2 * (kBlock / kWave))));
    dim3 grid(pb::div_up(nwave, kBlock), nwalkers);
    k_two_stream_net_batch<<<grid, kBlock, lds, pb::as_stream(stream)>>>(
        flux_d, parts_d, ec_d, intervals_d, wn_d, trapz_weights_d, temps_d, f_int_d, f_int_stride,
        flux_top_d, flux_top_stride, work_d, nlayers, nwave, pb_two_stream_net_parts(nwave));
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_radeq_update(const pb_radeq *state, int init_only, void *stream)
{
    PB_REQUIRE(state, "pb_radeq_update: null state struct");
    const pb_radeq &a = *state;
    PB_REQUIRE(a.nwalkers >= 0, "pb_radeq_update: %d profiles", a.nwalkers);
    const size_t lds = ((size_t)kRows * a.nlayers + 2 * kMaxRadius + 1 + kStage) * sizeof(double);
    PB_REQUIRE(a.nlayers >= 2 && a.nlayers <= PB_ATM_MAX_LAYERS && lds <= 64 * 1024,
               "pb_radeq_update: 2-%d layers, not %d (the profile's vectors are kept in LDS)",
               PB_ATM_MAX_LAYERS, a.nlayers);
    if (a.nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(a.nrows >= 1 && a.nparts >= 0, "pb_radeq_update: %d history rows, %d parts",
               a.nrows, a.nparts);
    PB_REQUIRE(a.temp_d && a.iter_d && a.pressure_d && a.vmr_d && a.dens_d && a.tab_map_d,
               "pb_radeq_update: null pointer");
    PB_REQUIRE(init_only || (a.temps_d && a.dt_scale_d && a.signs_d && a.q_up_d && a.q_down_d &&
                             a.dpress_d && (a.parts_d || a.nparts == 0)),
               "pb_radeq_update: null pointer");
    PB_REQUIRE(a.nspecies >= 1 && a.ntab >= 1 && a.ncont >= 0 &&
                   (a.ncont == 0 || (a.cont_map_d && a.cdens_d)),
               "pb_radeq_update: %d species, %d table species, %d continuum species", a.nspecies,
               a.ntab, a.ncont);
    PB_REQUIRE(a.vmr_stride == 0 || a.vmr_stride == (int64_t)a.nlayers * a.nspecies,
               "pb_radeq_update: the stride of vmr is 0 (shared) or nlayers * nspecies");
    PB_REQUIRE(a.rmodel >= -1 && a.rmodel <= 1,
               "pb_radeq_update: radius model %d (-1 fixed, 0 hydro_m, 1 hydro_g)", a.rmodel);
    if (a.rmodel >= 0) {
        PB_REQUIRE(a.lnp_d && a.mm_d && a.radius_d && a.intervals_d,
                   "pb_radeq_update: null pointer (radius model)");
        PB_REQUIRE(a.mm_stride == 0 || a.mm_stride == a.nlayers,
                   "pb_radeq_update: the stride of the mean mass is 0 (shared) or nlayers");
        PB_REQUIRE(a.rmodel == 1 || a.has_ref,
                   "pb_radeq_update: hydro_m needs a reference pressure and radius");
        if (a.has_ref)
            PB_REQUIRE(a.p0 > 0.0 && a.r0 > 0.0, "pb_radeq_update: p0 %g, r0 %g", a.p0, a.r0);
        if (a.rmodel == 0)
            PB_REQUIRE(a.mplanet > 0.0, "pb_radeq_update: mplanet %g", a.mplanet);
        else
            PB_REQUIRE(a.gplanet > 0.0, "pb_radeq_update: gplanet %g", a.gplanet);
    }
    k_radeq_update<<<a.nwalkers, kUpdate, lds, pb::as_stream(stream)>>>(a, init_only);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
