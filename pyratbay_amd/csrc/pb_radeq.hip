// Radiative equilibrium on the device (Pyrat.radiative_equilibrium, pyrat/pyrat_obj.py:559-646 ->
// spectrum/radiative_transfer.py:141-272) for a batch of profiles at fixed volume mixing ratios,
// with or without convection.  One iteration is three launches and no host work: the
// interpolation of the table (pb_interp_ec_batch[_cont]), k_two_stream_net_batch and
// k_radeq_update.
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
//
// k_radeq_update<true> (pb_radeq_update_convective) is the same kernel with the second half of the
// reference's loop (radiative_transfer.py:239-272) between the update and the atmosphere: the heat
// capacity of the caller's cp/R table at the temperatures the radiative half produced, the
// mixing-length flux of spectrum/convection.py:49-65, one workgroup-wide test whether any layer
// convects, and where one does the update again from Q_net + conv_flux.  Both halves are ONE
// function (update_from_flux); the first one of the convective kernel leaves the state it reads
// -- dt_scale, the sign row of this iteration -- unwritten until the outcome is known.
//
// With pb_radeq.temps_only the kernel ends behind the new temperatures: the loop that
// re-equilibrates the chemistry every iteration (pb_radeq_equilibrium, pb_chemistry.hip) forms the
// atmosphere in a launch of its own, init_only, once the VMRs are those of the new temperatures.
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
constexpr int kRowsConvection = 8;                   // ... with Q_net kept and the convective flux
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
using pb::wave_sum;

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

// Qup, Qdown of profile w: the parts in the order of part_groups, stored, and Q_net into s_q
// (every thread its own layers l = tid, tid + kUpdate, ...; no barrier behind them).  s_part: the
// groups' partial sums.
__device__ void sum_parts(const pb_radeq &a, int64_t w, double *s_q, double *s_part)
{
    const int L = a.nlayers;
    const int tid = threadIdx.x;
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
}

// The profile-length vectors of the update in LDS
struct Rows {
    double *t;                        // T of this iteration
    double *q;                        // Q_net; |dT|; the hydrostatic integrand
    double *df;                       // dF; the cumulative hydrostatic integral
    double *a;                        // dt_scale_tmp before its filter; T of the next iteration
    double *b;                        // dt_scale_tmp; the radius
    double *tn;                       // T + dT
    double *w;                        // [2 kMaxRadius + 1] filter weights
    double *qn, *cf;                  // (k_radeq_update<true>) Q_net kept; the convective flux
    int *radius;                      // the radius of the temperature filter
};

// The update from a net flux s_f (radiative_transfer.py:211-233, and 254-272 with the convective
// flux added): s_f may be s.q.  Writes row k + 1 of the history, temp_d and the diagnostics, and
// leaves the next profile in s.a and the new dt_scale in s.b, behind a barrier; the state the
// statements read -- row k % 4 of the signs, dt_scale_d -- is written only with commit.
__device__ void update_from_flux(const pb_radeq &a, int64_t w, int k, const double *s_f,
                                 const Rows &s, bool commit)
{
    const int L = a.nlayers;
    const int tid = threadIdx.x;
    if (tid == 0)
        gauss_weights(1.5, s.w);
    __syncthreads();
    // dF, its sign, the wobbling layers, dt_scale_tmp before the filter
    const int nprev = min(k, 4);
    for (int l = tid; l < L; l += kUpdate) {
        const double dF = l == 0 ? 0.0 : s_f[l] - s_f[l - 1];
        const double sg = np_sign(dF);
        bool wobble = false;
        for (int r = 1; r <= nprev; r++)
            if ((a.signs_d[(w * 4 + ((k - r) & 3)) * L + l] - sg) != 0.0)
                wobble = true;
        if (commit)
            a.signs_d[(w * 4 + (k & 3)) * L + l] = sg;
        if (a.wobble_d)
            a.wobble_d[w * L + l] = wobble;
        double v = a.dt_scale_d[w * L + l] * (wobble ? 0.5 : 1.15);
        v = v < 1.0 ? 1.0 : v;                   // np.clip = minimum(maximum(x, lo), hi)
        v = v > 1.0e8 ? 1.0e8 : v;
        s.df[l] = dF;
        s.a[l] = v;
    }
    __syncthreads();
    for (int l = tid; l < L; l += kUpdate) {
        const double dts = correlate_reflect(s.a, l, L, s.w, 6);
        const double dF = s.df[l], t = s.t[l];
        const double dT = ((dts * np_sign(dF)) * pow(fabs(dF), 0.1)) /
                          ((kSigmaSB * pow(t, 3.0)) * a.dpress_d[l]);
        s.b[l] = dts;
        s.tn[l] = t + dT;
        s.q[l] = fabs(dT);
    }
    __syncthreads();
    if (tid == 0) {
        s.tn[0] = s.tn[1];                       // isothermal top
        double sigma = (np_sum<4>(s.q, L) / (double)L) / 10.0;
        sigma = sigma < 0.75 ? 0.75 : sigma;
        sigma = sigma > 2.0 ? 2.0 : sigma;
        *s.radius = gauss_weights(sigma, s.w);
        a.iter_d[w] = k + 1;
        if (a.sigma_d)
            a.sigma_d[w] = sigma;
    }
    __syncthreads();
    const int radius = *s.radius;
    for (int l = tid; l < L; l += kUpdate) {
        double v = l < L - 1 ? correlate_reflect(s.tn, l, L, s.w, radius) : s.tn[l];
        v = v < a.tmin ? a.tmin : v;
        v = v > a.tmax ? a.tmax : v;
        s.a[l] = v;
        if (commit)
            a.dt_scale_d[w * L + l] = s.b[l];
        a.temps_d[(w * a.nrows + k + 1) * L + l] = v;
        a.temp_d[w * L + l] = v;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------- the convective half

constexpr double kAmu = 1.66053906892e-27 * 1e3;     // pc.amu = sc 'unified atomic mass unit' * 1e3

// np_sum_block of the n values f(0 .. n - 1), n <= 128
template <class F>
__device__ __forceinline__ double np_sum_of(int n, F f)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; i++)
            res += f(i);
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; j++)
        r[j] = f(j);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++)
            r[j] += f(i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++)
        res += f(i);
    return res;
}

// np.interp(x, xp[n], fp[n * stride : stride]): interp_clamped of pb_clouds.hip on one column of a
// table (the end values outside it, the node's own value on a node)
__device__ inline double interp_column(const double *xp, const double *fp, int stride, int n,
                                       double x)
{
    if (x > xp[n - 1])
        return fp[(int64_t)(n - 1) * stride];
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
    const double f0 = fp[(int64_t)lo * stride];
    if (lo == n - 1 || xp[lo] == x)
        return f0;
    const double slope = (fp[(int64_t)(lo + 1) * stride] - f0) / (xp[lo + 1] - xp[lo]);
    return slope * (x - xp[lo]) + f0;
}

// convection.convective_flux (spectrum/convection.py:49-65) at one layer: grad_t = the
// logarithmic gradient of the temperature over convection.py's own dpress, coeff =
// alpha**2 sqrt(beta); the product left to right
__device__ inline double convective_flux(double coeff, double grad_t, double temp, double cp,
                                         double gravity, double mu, double rho)
{
    const double cv = cp - pb::atm::kBoltz / kAmu;
    const double gamma = cp / cv;
    const double grad_ad = 1.0 - 1.0 / gamma;
    double delta = grad_t - grad_ad;
    delta = delta < 0.0 ? 0.0 : delta;           // np.clip(x, 0, inf): a NaN stays
    const double H = (pb::atm::kBoltz * temp) / ((mu * kAmu) * gravity);
    return ((((coeff * cp) / mu) * rho) * temp) * sqrt(gravity * H) * pow(delta, 1.5);
}

// radiative_transfer.py:239-272 behind update_from_flux(.., commit = false): the heat capacity and
// the convective flux at the temperatures the radiative half left in s.a, with the gravity,
// density and mean mass of the evaluated profile (s.t, radius_d as it is on entry); where a layer
// convects, the update again from Q_net + conv_flux; else the radiative half's state is written.
__device__ void convective_half(const pb_radeq &a, const pb_radeq_convection &c, int64_t w, int k,
                                const Rows &s)
{
    const int L = a.nlayers, S = a.nspecies;
    const int tid = threadIdx.x;
    const double *vmr = a.vmr_d + w * a.vmr_stride;
    const double *mm = a.mm_d + w * a.mm_stride;
    const double *cp_table = c.cp_table_d + w * c.cp_table_stride;
    int nonzero = 0;
    for (int l = tid; l < L; l += kUpdate) {
        const double tn = s.a[l], tk = s.t[l], p = a.pressure_d[l];
        const double *x = vmr + (int64_t)l * S;
        const double cp = (np_sum_of(S, [&](int j) {
            return interp_column(c.cp_temps_d, cp_table + j, S, c.ntemps, tn) * x[j];
        }) * pb::atm::kBoltz) / kAmu;
        const double r = a.radius_d[w * L + l];
        const double gravity = (pb::atm::kGrav * c.mplanet) / (r * r);
        const double rho = np_sum_of(S, [&](int j) {
            return pb::atm::ideal_gas_density(x[j], p, tk) * c.mol_mass_d[j];
        }) * kAmu;
        const double grad_t = (l == 0 ? 0.0 : log(tn) - log(s.a[l - 1])) / c.conv_dpress_d[l];
        const double f = convective_flux(c.coeff, grad_t, tn, cp, gravity, mm[l], rho);
        s.cf[l] = f;
        c.conv_flux_d[w * L + l] = f;
        nonzero |= !(f == 0.0);                  // (a NaN is not zero)
    }
    const int convective = __syncthreads_or(nonzero) != 0;
    if (tid == 0)
        c.convective_d[w] = convective;
    if (!convective) {
        // np.all(conv_flux == 0): the radiative result stands
        for (int l = tid; l < L; l += kUpdate) {
            a.signs_d[(w * 4 + (k & 3)) * L + l] = np_sign(s.df[l]);
            a.dt_scale_d[w * L + l] = s.b[l];
        }
        return;
    }
    for (int l = tid; l < L; l += kUpdate)
        s.qn[l] = s.qn[l] + s.cf[l];
    update_from_flux(a, w, k, s.qn, s, true);        // (begins with a barrier)
}

// kConv: pb_radeq_update_convective (two more rows; c is not read otherwise)
template <bool kConv>
__global__ __launch_bounds__(kUpdate) void k_radeq_update(pb_radeq a, pb_radeq_convection c,
                                                          int init_only)
{
    extern __shared__ double s_row[];
    const int L = a.nlayers;
    const int tid = threadIdx.x;
    const int64_t w = blockIdx.x;
    __shared__ int s_radius;
    Rows s;
    s.t = s_row;
    s.q = s.t + L;
    s.df = s.q + L;
    s.a = s.df + L;
    s.b = s.a + L;
    s.tn = s.b + L;
    s.qn = s.tn + L;
    s.cf = s.qn + L;
    s.w = s.tn + (kConv ? 3 : 1) * L;
    s.radius = &s_radius;
    // the groups' partial sums [groups][2][L]: groups * L <= kUpdate up to kUpdate layers, i.e. at
    // most kStage doubles behind the weights; above that ONE group, 2 L doubles, which lie over
    // s.a and s.b (both dead until the sums have been read, a barrier before their first store)
    double *s_part = L > kUpdate ? s.a : s.w + 2 * kMaxRadius + 1;
    const int k = a.iter_d[w];
    // (a launch beyond the rows of the history does nothing)
    if (!init_only && (k < 0 || k + 1 >= a.nrows))
        return;
    for (int l = tid; l < L; l += kUpdate)
        s.t[l] = a.temp_d[w * L + l];
    double *s_next = s.t;
    if (!init_only) {
        sum_parts(a, w, s.q, s_part);
        if (kConv)
            for (int l = tid; l < L; l += kUpdate)
                s.qn[l] = s.q[l];
        update_from_flux(a, w, k, s.q, s, !kConv);
        if (kConv)
            convective_half(a, c, w, k, s);
        // (the caller re-equilibrates the VMRs at the new temperatures first, then asks for the
        // atmosphere with init_only)
        if (a.temps_only)
            return;
        s_next = s.a;
    } else {
        __syncthreads();
    }
    double *s_q = s.q, *s_df = s.df, *s_b = s.b;
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

// The most layers whose `rows` vectors fit 64 KiB of LDS beside the weights and the partial sums:
// PB_ATM_MAX_LAYERS with the 6 rows of pb_radeq_update, 957 with the 8 of
// pb_radeq_update_convective ((8192 - 17 - 512) / 8 doubles)
constexpr int max_layers_of(int rows)
{
    const int fit = (64 * 1024 / (int)sizeof(double) - (2 * kMaxRadius + 1) - kStage) / rows;
    return fit < PB_ATM_MAX_LAYERS ? fit : PB_ATM_MAX_LAYERS;
}
static_assert(max_layers_of(kRowsConvection) == 957, "pbhip.h and radeq.py state this limit");

// The checks both entries of the update make before their launch; *lds_bytes: the dynamic LDS of
// `rows` profile-length vectors, the filter weights and the groups' partial sums.
int check_update(const pb_radeq &a, int init_only, const char *name, int rows, size_t *lds_bytes)
{
    const int max_layers = max_layers_of(rows);
    PB_REQUIRE(a.nwalkers >= 0, "%s: %d profiles", name, a.nwalkers);
    const size_t lds = ((size_t)rows * a.nlayers + 2 * kMaxRadius + 1 + kStage) * sizeof(double);
    PB_REQUIRE(a.nlayers >= 2 && a.nlayers <= max_layers,
               "%s: 2-%d layers, not %d (the profile's vectors are kept in LDS)", name,
               max_layers, a.nlayers);
    *lds_bytes = lds;
    if (a.nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(a.nrows >= 1 && a.nparts >= 0, "%s: %d history rows, %d parts", name,
               a.nrows, a.nparts);
    PB_REQUIRE(a.temp_d && a.iter_d && a.pressure_d && a.vmr_d && a.dens_d && a.tab_map_d,
               "%s: null pointer", name);
    PB_REQUIRE(init_only || (a.temps_d && a.dt_scale_d && a.signs_d && a.q_up_d && a.q_down_d &&
                             a.dpress_d && (a.parts_d || a.nparts == 0)),
               "%s: null pointer", name);
    PB_REQUIRE(a.nspecies >= 1 && a.ntab >= 1 && a.ncont >= 0 &&
                   (a.ncont == 0 || (a.cont_map_d && a.cdens_d)),
               "%s: %d species, %d table species, %d continuum species", name, a.nspecies,
               a.ntab, a.ncont);
    PB_REQUIRE(a.vmr_stride == 0 || a.vmr_stride == (int64_t)a.nlayers * a.nspecies,
               "%s: the stride of vmr is 0 (shared) or nlayers * nspecies", name);
    PB_REQUIRE(a.rmodel >= -1 && a.rmodel <= 1,
               "%s: radius model %d (-1 fixed, 0 hydro_m, 1 hydro_g)", name, a.rmodel);
    if (a.rmodel >= 0) {
        PB_REQUIRE(a.lnp_d && a.mm_d && a.radius_d && a.intervals_d,
                   "%s: null pointer (radius model)", name);
        PB_REQUIRE(a.mm_stride == 0 || a.mm_stride == a.nlayers,
                   "%s: the stride of the mean mass is 0 (shared) or nlayers", name);
        PB_REQUIRE(a.rmodel == 1 || a.has_ref,
                   "%s: hydro_m needs a reference pressure and radius", name);
        if (a.has_ref)
            PB_REQUIRE(a.p0 > 0.0 && a.r0 > 0.0, "%s: p0 %g, r0 %g", name, a.p0, a.r0);
        if (a.rmodel == 0)
            PB_REQUIRE(a.mplanet > 0.0, "%s: mplanet %g", name, a.mplanet);
        else
            PB_REQUIRE(a.gplanet > 0.0, "%s: gplanet %g", name, a.gplanet);
    }
    return PB_OK;
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
    size_t lds = 0;
    const int rc = check_update(a, init_only, "pb_radeq_update", kRows, &lds);
    if (rc != PB_OK || a.nwalkers == 0)
        return rc;
    k_radeq_update<false><<<a.nwalkers, kUpdate, lds, pb::as_stream(stream)>>>(
        a, pb_radeq_convection{}, init_only);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_radeq_update_convective(const pb_radeq *state, const pb_radeq_convection *conv, void *stream)
{
    PB_REQUIRE(state && conv, "pb_radeq_update_convective: null state or convection struct");
    const pb_radeq &a = *state;
    const pb_radeq_convection &c = *conv;
    size_t lds = 0;
    const int rc = check_update(a, 0, "pb_radeq_update_convective", kRowsConvection, &lds);
    if (rc != PB_OK || a.nwalkers == 0)
        return rc;
    PB_REQUIRE(c.cp_temps_d && c.cp_table_d && c.mol_mass_d && c.conv_dpress_d && c.conv_flux_d &&
                   c.convective_d && a.mm_d && a.radius_d,
               "pb_radeq_update_convective: null pointer (convection)");
    PB_REQUIRE(c.ntemps >= 1, "pb_radeq_update_convective: %d temperatures in the heat-capacity "
               "table", c.ntemps);
    PB_REQUIRE(c.cp_table_stride == 0 || c.cp_table_stride == (int64_t)c.ntemps * a.nspecies,
               "pb_radeq_update_convective: the stride of the heat-capacity table is 0 (shared) or "
               "ntemps * nspecies");
    PB_REQUIRE(a.nspecies <= 128, "pb_radeq_update_convective: %d species: at most 128 (one block "
               "of NumPy's pairwise sum)", a.nspecies);
    PB_REQUIRE(a.mm_stride == 0 || a.mm_stride == a.nlayers,
               "pb_radeq_update_convective: the stride of the mean mass is 0 (shared) or nlayers");
    PB_REQUIRE(c.mplanet > 0.0 && c.coeff == c.coeff,
               "pb_radeq_update_convective: mplanet %g, coeff %g", c.mplanet, c.coeff);
    PB_REQUIRE(a.rmodel != 1 || a.has_ref, "pb_radeq_update_convective: hydro_g without a "
               "reference radius has radius 0 at the bottom: no gravity there");
    k_radeq_update<true><<<a.nwalkers, kUpdate, lds, pb::as_stream(stream)>>>(a, c, 0);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
