// Batched multi-start Levenberg-Marquardt for the retrieval loop: the residual vector of a walker
// batch, the finite-difference probe points, the normal equations J^T J / J^T R of every start,
// the damped Cholesky solves of the trial steps, the accept / reject decision and the Laplace
// covariance.  pyratbay_amd/optimize.py states every kernel in NumPy (the specification).
//
// Reproducible by construction: no atomics on doubles; every sum has one fixed order --
//   * an element of J^T J and of J^T R is summed over the data points in index order by ONE thread;
//   * a cost 0.5 |R|^2 is summed in 64 lane-strided partial sums (lane j: i = j, j + 64, ...), then
//     the xor butterfly 32, 16, ..., 1 (pb::wave_sum), in pb_lm_normal and pb_lm_update alike.
#include "pb_common.h"

namespace {

constexpr int kMaxParams = PB_RETRIEVAL_MAX_PARAMS;     // 128
constexpr int kTile = 32;          // a block of pb_lm_normal owns a 32 x 32 tile of A
constexpr int kChunk = PB_LM_CHUNK;   // 64 data points staged in LDS per step of the m loop
constexpr int kPad = kChunk + 1;   // row stride of the staged columns: lanes of a half wave read
                                   // 16 distinct columns, 2 * 65 * col mod 64 banks: no conflict
constexpr int kNormalBlock = 256;
constexpr int kSolveBlock = 256;

enum { RUNNING = 0, GTOL = 1, FTOL = 2, XTOL = 3, STALL = 4, MAXIT = 5 };

__device__ __forceinline__ bool finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// ---------------------------------------------------------------------------
// residuals[w, m], m = ndata + ngauss.  One block per walker: a first pass decides whether the
// walker is rejected (outside the bounds, or a non-finite band flux), the second writes the row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lm_residuals(
    double *out, const double *model, const double *data, const double *uncert,
    const int32_t *offset_group, const double *offset_vals, double offset_unit, int noff,
    const int32_t *err_group, const int32_t *err_mode, const double *err_vals, double err_unit,
    int nerr, const double *theta, const int32_t *inside, const int32_t *gauss_index,
    const double *prior, const double *priorlow, const double *priorup, int ngauss, int nfree,
    int ndata)
{
    const int w = blockIdx.x;
    const double *mrow = model + (int64_t)w * ndata;
    double *row = out + (int64_t)w * ((int64_t)ndata + ngauss);
    int bad = inside[w] == 0;
    for (int b = threadIdx.x; b < ndata && !bad; b += 256)
        bad = !finite(mrow[b]);
    bad = __syncthreads_or(bad);
    if (bad) {
        for (int i = threadIdx.x; i < ndata + ngauss; i += 256)
            row[i] = INFINITY;
        return;
    }
    const double *ov = noff ? offset_vals + (int64_t)w * noff : nullptr;
    const double *ev = nerr ? err_vals + (int64_t)w * nerr : nullptr;
    for (int b = threadIdx.x; b < ndata; b += 256) {
        double d = data[b], u = uncert[b];
        if (ov) {
            const int g = offset_group[b];
            if (g >= 0 && g < noff)
                d = d + ov[g] * offset_unit;
        }
        if (ev) {
            const int g = err_group[b];
            if (g >= 0 && g < nerr) {
                double e = pow(10.0, ev[g]);
                if (err_mode[g] == 0) {
                    u = u * e;
                } else {
                    e *= err_unit;
                    u = sqrt(u * u + e * e);
                }
            }
        }
        row[b] = (d - mrow[b]) / u;
    }
    for (int j = threadIdx.x; j < ngauss; j += 256) {
        const int k = gauss_index[j];
        double r = INFINITY;
        if (k >= 0 && k < nfree) {
            const double p = theta[(int64_t)w * nfree + k];
            const double s = p < prior[k] ? priorlow[k] : priorup[k];
            r = (p - prior[k]) / s;
        }
        row[ndata + j] = r;
    }
}

// ---------------------------------------------------------------------------
// probe[s, 0] = theta[s]; probe[s, k + 1] = theta[s] + hs e_k, hs = +h_k, or -h_k where
// theta_k + h_k > pmax_k; h_k = fd_step * scale_k.  step[s, k] = hs.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lm_probe(double *probe, double *step, const double *theta,
                                                  const double *pmax, const double *scale,
                                                  double fd_step, int nfree, int64_t total)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total)
        return;
    const int f = (int)(e % nfree);
    const int64_t q = e / nfree;
    const int r = (int)(q % (nfree + 1));
    const int64_t s = q / (nfree + 1);
    double v = theta[s * nfree + f];
    if (r == f + 1) {
        const double h = fd_step * scale[f];
        const double hs = (v + h > pmax[f]) ? -h : h;
        v = v + hs;
        step[s * nfree + f] = hs;
    }
    probe[e] = v;
}

// ---------------------------------------------------------------------------
// A[s] = J^T J, g[s] = J^T R_0, cost[s] = 0.5 |R_0|^2 with J_ik = (R[s, k+1, i] - R[s, 0, i]) / hs_k.
// Block = (start, tile (bk <= bl) of the upper triangle), 256 threads, 2 x 2 elements each:
// S_kl = sum_i D_ik D_il in index order with D = the differences, staged through LDS kChunk points
// at a time; A_kl = (S_kl / hs_min(k,l)) / hs_max(k,l), written to (k, l) and (l, k): symmetric in
// bits.  The diagonal tiles also sum g (threads 0..31, one column each); tile (0, 0) sums the
// cost (wavefront 1).  A column with a non-finite difference is frozen: its row and column of A
// and its g are 0.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kNormalBlock) void k_lm_normal(
    double *A, double *g, double *cost, const double *R, const double *step, int nfree, int m,
    int ntiles)
{
    __shared__ double s_k[kTile * kPad];
    __shared__ double s_l[kTile * kPad];
    __shared__ double s_r0[kChunk];
    __shared__ int s_bad[2 * kTile];

    const int64_t s = blockIdx.x / ntiles;
    int t = blockIdx.x % ntiles, bk = 0;
    // tile t of the upper triangle, row by row: (0,0) (0,1) .. (0,T-1) (1,1) ..
    const int T = (nfree + kTile - 1) / kTile;
    while (t >= T - bk) {
        t -= T - bk;
        bk++;
    }
    const int bl = bk + t;
    const bool diag = bk == bl;
    const int k0 = bk * kTile, l0 = bl * kTile;
    const int tid = threadIdx.x;
    const int tk = tid >> 4, tl = tid & 15;        // rows 2 tk, 2 tk + 1; columns 2 tl, 2 tl + 1
    const double *Rs = R + s * (int64_t)(nfree + 1) * m;

    if (tid < 2 * kTile)
        s_bad[tid] = 0;
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0, gk = 0.0, c = 0.0;
    const int lane_i = tid & (kChunk - 1), col0 = tid >> 6;      // staging: 4 columns per pass
    for (int i0 = 0; i0 < m; i0 += kChunk) {
        const int n = min(kChunk, m - i0);
        __syncthreads();
        {
            const bool in = lane_i < n;
            const double r0 = in ? Rs[i0 + lane_i] : 0.0;
            if (col0 == 0)
                s_r0[lane_i] = r0;
            for (int cc = col0; cc < kTile; cc += kNormalBlock / kChunk) {
                const int k = k0 + cc, l = l0 + cc;
                double dk = 0.0, dl = 0.0;
                if (in && k < nfree) {
                    dk = Rs[(int64_t)(k + 1) * m + i0 + lane_i] - r0;
                    if (!finite(dk))
                        s_bad[cc] = 1;
                }
                s_k[cc * kPad + lane_i] = dk;
                if (!diag) {
                    if (in && l < nfree) {
                        dl = Rs[(int64_t)(l + 1) * m + i0 + lane_i] - r0;
                        if (!finite(dl))
                            s_bad[kTile + cc] = 1;
                    }
                    s_l[cc * kPad + lane_i] = dl;
                }
            }
        }
        __syncthreads();
        const double *pk = s_k + (2 * tk) * kPad;
        const double *pl = (diag ? s_k : s_l) + (2 * tl) * kPad;
        for (int i = 0; i < n; i++) {
            const double x0 = pk[i], x1 = pk[kPad + i];
            const double y0 = pl[i], y1 = pl[kPad + i];
            a00 += x0 * y0;
            a01 += x0 * y1;
            a10 += x1 * y0;
            a11 += x1 * y1;
        }
        if (diag && tid < kTile) {
            const double *p = s_k + tid * kPad;
            for (int i = 0; i < n; i++)
                gk += p[i] * s_r0[i];
        }
        if (blockIdx.x % ntiles == 0 && (tid >> 6) == 1 && lane_i < n)
            c += s_r0[lane_i] * s_r0[lane_i];
    }
    __syncthreads();
    const double *hs = step + s * nfree;
    double *As = A + s * (int64_t)nfree * nfree;
    const double acc[2][2] = {{a00, a01}, {a10, a11}};
#pragma unroll
    for (int a = 0; a < 2; a++) {
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int ck = 2 * tk + a, cl = 2 * tl + b;
            const int k = k0 + ck, l = l0 + cl;
            if (k >= nfree || l >= nfree)
                continue;
            const bool frozen = s_bad[ck] || s_bad[diag ? cl : kTile + cl];
            const int lo = min(k, l), hi = max(k, l);
            const double v = frozen ? 0.0 : (acc[a][b] / hs[lo]) / hs[hi];
            As[(int64_t)k * nfree + l] = v;
            if (!diag)
                As[(int64_t)l * nfree + k] = v;
        }
    }
    if (diag && tid < kTile && k0 + tid < nfree)
        g[s * nfree + k0 + tid] = s_bad[tid] ? 0.0 : gk / hs[k0 + tid];
    if (blockIdx.x % ntiles == 0 && (tid >> 6) == 1) {
        c = pb::wave_sum(c);
        if (lane_i == 0)
            cost[s] = 0.5 * c;
    }
}

// ---------------------------------------------------------------------------
// The free set of a start, in index order, into LDS: k is active (left out) if it sits on a bound
// with the gradient pushing outward, or A_kk == 0.  One thread; nfree <= 128.
// ---------------------------------------------------------------------------
__device__ int free_set(int *s_free, int32_t *active_out, const double *A, const double *g,
                        const double *theta, const double *pmin, const double *pmax, int nfree)
{
    int nf = 0;
    for (int k = 0; k < nfree; k++) {
        const double gk = g[k], tkv = theta[k];
        const bool act = (tkv <= pmin[k] && gk > 0.0) || (tkv >= pmax[k] && gk < 0.0) ||
                         A[(int64_t)k * nfree + k] == 0.0;
        if (active_out)
            active_out[k] = act;
        if (!act)
            s_free[nf++] = k;
    }
    return nf;
}

// In-place right-looking Cholesky of the lower triangle of M[nf, nf] (row stride ld, global
// memory owned by this block).  -> 0, or 1 at the first pivot that is not finite or not above
// tol d0[p], d0 the diagonal before the factorisation (tol == 0: a pivot <= 0).
__device__ int cholesky(double *M, int nf, int ld, double tol, const double *d0)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int p = 0; p < nf; p++) {
        __syncthreads();
        const double d = M[(int64_t)p * ld + p];
        const double least = tol > 0.0 ? tol * d0[p] : 0.0;
        if (!(d > least) || !finite(d))
            return 1;                                   // (block-uniform)
        const double lpp = sqrt(d);
        __syncthreads();
        if (tid == 0)
            M[(int64_t)p * ld + p] = lpp;
        for (int a = p + 1 + tid; a < nf; a += nt)
            M[(int64_t)a * ld + p] = M[(int64_t)a * ld + p] / lpp;
        __syncthreads();
        const int rest = nf - p - 1;
        for (int e = tid; e < rest * rest; e += nt) {
            const int a = p + 1 + e / rest, b = p + 1 + e % rest;
            if (b <= a)
                M[(int64_t)a * ld + b] =
                    M[(int64_t)a * ld + b] - M[(int64_t)a * ld + p] * M[(int64_t)b * ld + p];
        }
    }
    __syncthreads();
    return 0;
}

// ---------------------------------------------------------------------------
// Block = (start, trial j): (A_ff + lam_j diag(A_ff)) delta = -g_f by Cholesky in work[s, j],
// lam_j = lam nu^(j-1) (lam / nu, then times nu per trial); trial = clip(theta + delta, pmin, pmax);
// a failed pivot: trial = theta.  Trial 0 also writes pgrad[s] = max over free k of |g_k| scale_k.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kSolveBlock) void k_lm_step(
    double *trial, double *pgrad, double *work, const double *A, const double *g,
    const double *theta, const double *lam, const double *pmin, const double *pmax,
    const double *scale, double nu, int ntrial, int nfree)
{
    __shared__ int s_free[kMaxParams];
    __shared__ double s_b[kMaxParams];
    __shared__ int s_nf;
    const int64_t s = blockIdx.x / ntrial;
    const int j = blockIdx.x % ntrial;
    const int tid = threadIdx.x, nt = blockDim.x;
    const double *As = A + s * (int64_t)nfree * nfree;
    const double *gs = g + s * nfree, *th = theta + s * nfree;
    double *out = trial + (s * ntrial + j) * (int64_t)nfree;
    double *M = work + (s * ntrial + j) * (int64_t)nfree * nfree;

    if (tid == 0)
        s_nf = free_set(s_free, nullptr, As, gs, th, pmin, pmax, nfree);
    for (int k = tid; k < nfree; k += nt)
        out[k] = th[k];
    __syncthreads();
    const int nf = s_nf;
    if (j == 0 && tid == 0) {
        double pg = 0.0;
        for (int a = 0; a < nf; a++)
            pg = fmax(pg, fabs(gs[s_free[a]]) * scale[s_free[a]]);
        pgrad[s] = pg;
    }
    if (nf == 0)
        return;
    double lj = lam[s] / nu;
    for (int q = 0; q < j; q++)
        lj = lj * nu;
    for (int e = tid; e < nf * nf; e += nt) {
        const int a = e / nf, b = e % nf;
        if (b > a)
            continue;
        double v = As[(int64_t)s_free[a] * nfree + s_free[b]];
        if (a == b)
            v = v + lj * v;
        M[(int64_t)a * nfree + b] = v;
    }
    for (int a = tid; a < nf; a += nt)
        s_b[a] = -gs[s_free[a]];
    if (cholesky(M, nf, nfree, 0.0, nullptr))
        return;                                         // trial stays theta
    // L y = b (column by column), then L^T delta = y
    for (int p = 0; p < nf; p++) {
        __syncthreads();
        const double y = s_b[p] / M[(int64_t)p * nfree + p];
        __syncthreads();
        if (tid == 0)
            s_b[p] = y;
        for (int a = p + 1 + tid; a < nf; a += nt)
            s_b[a] = s_b[a] - M[(int64_t)a * nfree + p] * y;
    }
    for (int p = nf - 1; p >= 0; p--) {
        __syncthreads();
        const double d = s_b[p] / M[(int64_t)p * nfree + p];
        __syncthreads();
        if (tid == 0)
            s_b[p] = d;
        for (int a = tid; a < p; a += nt)
            s_b[a] = s_b[a] - M[(int64_t)p * nfree + a] * d;
    }
    __syncthreads();
    // a non-finite step (an overflow on the way) is a failure like a bad pivot
    int bad = 0;
    for (int a = tid; a < nf; a += nt)
        bad |= !finite(s_b[a]);
    if (__syncthreads_or(bad))
        return;
    for (int a = tid; a < nf; a += nt) {
        const int k = s_free[a];
        out[k] = fmin(fmax(th[k] + s_b[a], pmin[k]), pmax[k]);
    }
}

// ---------------------------------------------------------------------------
// One wavefront per start: the trial costs, the pick, accept / reject, lambda and the status
// (optimize.py: update_host).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_lm_update(
    double *theta, double *cost, double *lam, int32_t *status, int32_t *niter, int32_t *picked,
    const double *trial, const double *Rt, const double *pgrad, const double *scale, double nu,
    double lam_min, double lam_max, double gtol, double ftol, double xtol, int max_iter,
    int ntrial, int nfree, int m)
{
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    if (status[s] != RUNNING)
        return;                                         // (wave-uniform)
    const double c0 = cost[s];
    if (!finite(c0) || pgrad[s] <= gtol) {
        if (lane == 0) {
            status[s] = finite(c0) ? GTOL : STALL;
            picked[s] = -1;
        }
        return;
    }
    int best = -1;
    double cbest = INFINITY;
    for (int j = 0; j < ntrial; j++) {
        const double *r = Rt + (s * ntrial + j) * (int64_t)m;
        double c = 0.0;
        for (int i = lane; i < m; i += 64)
            c += r[i] * r[i];
        c = 0.5 * pb::wave_sum(c);
        if (finite(c) && c < cbest) {
            cbest = c;
            best = j;
        }
    }
    const double l0 = lam[s];
    int st = RUNNING;
    double lnew;
    if (best >= 0 && cbest < c0) {
        const double *tr = trial + (s * ntrial + best) * (int64_t)nfree;
        double dx = 0.0;
        for (int k = lane; k < nfree; k += 64) {
            const double t0 = theta[s * nfree + k];
            dx = fmax(dx, fabs(tr[k] - t0) / scale[k]);
            theta[s * nfree + k] = tr[k];
        }
        for (int off = 32; off > 0; off >>= 1)
            dx = fmax(dx, __shfl_xor(dx, off));
        double lj = l0 / nu;
        for (int q = 0; q < best; q++)
            lj = lj * nu;
        lnew = fmax(lj / nu, lam_min);
        if (c0 - cbest <= ftol * fmax(c0, 1.0))
            st = FTOL;
        else if (dx <= xtol)
            st = XTOL;
        if (lane == 0)
            cost[s] = cbest;
    } else {
        best = -1;
        lnew = l0;
        for (int q = 0; q < ntrial; q++)
            lnew = lnew * nu;
    }
    if (lane == 0) {
        const int it = niter[s] + 1;
        if (st == RUNNING && lnew > lam_max)
            st = STALL;
        if (st == RUNNING && it >= max_iter)
            st = MAXIT;
        lam[s] = lnew;
        niter[s] = it;
        status[s] = st;
        picked[s] = best;
    }
}

// unfinished[0] = how many starts are still running.  One block, integer sums.
__global__ __launch_bounds__(256) void k_lm_count(int32_t *unfinished, const int32_t *status,
                                                  int64_t ns)
{
    __shared__ int s_n[256];
    int n = 0;
    for (int64_t s = threadIdx.x; s < ns; s += 256)
        n += status[s] == RUNNING;
    s_n[threadIdx.x] = n;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            s_n[threadIdx.x] += s_n[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        unfinished[0] = s_n[0];
}

// ---------------------------------------------------------------------------
// C[s] = inverse of A_ff on the free set of the start (free_set), 0 in the active rows and
// columns.  Cholesky in work[s]; then thread c solves L L^T x = e_c on its own; the upper triangle
// of the result is mirrored, so that C is symmetric in bits.  Numerically singular (a pivot not
// above nf eps A_pp): NaN in the free block and singular[s] = 1.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kSolveBlock) void k_lm_covariance(
    double *Cov, int32_t *active, int32_t *singular, double *work, const double *A,
    const double *g, const double *theta, const double *pmin, const double *pmax, int nfree)
{
    __shared__ int s_free[kMaxParams];
    __shared__ double s_d0[kMaxParams];
    __shared__ int s_nf;
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    const double *As = A + s * (int64_t)nfree * nfree;
    double *Cs = Cov + s * (int64_t)nfree * nfree;
    double *M = work + s * (int64_t)2 * nfree * nfree;
    double *X = M + (int64_t)nfree * nfree;

    if (tid == 0)
        s_nf = free_set(s_free, active + s * nfree, As, g + s * nfree, theta + s * nfree, pmin,
                        pmax, nfree);
    for (int e = tid; e < nfree * nfree; e += nt)
        Cs[e] = 0.0;
    __syncthreads();
    const int nf = s_nf;
    for (int e = tid; e < nf * nf; e += nt) {
        const int a = e / nf, b = e % nf;
        if (b <= a)
            M[(int64_t)a * nfree + b] = As[(int64_t)s_free[a] * nfree + s_free[b]];
    }
    for (int a = tid; a < nf; a += nt)
        s_d0[a] = As[(int64_t)s_free[a] * nfree + s_free[a]];
    // numerically singular: a pivot that the rounding of nf updates could have made
    const int fail = cholesky(M, nf, nfree, nf * 2.220446049250313e-16, s_d0);
    if (tid == 0)
        singular[s] = fail;
    if (fail) {
        for (int e = tid; e < nf * nf; e += nt)
            Cs[(int64_t)s_free[e / nf] * nfree + s_free[e % nf]] = NAN;
        return;
    }
    for (int c = tid; c < nf; c += nt) {
        // x[a] lives in X[a, c]; rows below c of the forward solve start at 0
        for (int a = 0; a < nf; a++)
            X[(int64_t)a * nfree + c] = a == c ? 1.0 : 0.0;
        for (int p = c; p < nf; p++) {
            const double y = X[(int64_t)p * nfree + c] / M[(int64_t)p * nfree + p];
            X[(int64_t)p * nfree + c] = y;
            for (int a = p + 1; a < nf; a++)
                X[(int64_t)a * nfree + c] =
                    X[(int64_t)a * nfree + c] - M[(int64_t)a * nfree + p] * y;
        }
        for (int p = nf - 1; p >= 0; p--) {
            const double d = X[(int64_t)p * nfree + c] / M[(int64_t)p * nfree + p];
            X[(int64_t)p * nfree + c] = d;
            for (int a = 0; a < p; a++)
                X[(int64_t)a * nfree + c] =
                    X[(int64_t)a * nfree + c] - M[(int64_t)p * nfree + a] * d;
        }
    }
    __syncthreads();
    for (int e = tid; e < nf * nf; e += nt) {
        const int a = e / nf, b = e % nf;
        const double v = X[(int64_t)min(a, b) * nfree + max(a, b)];
        Cs[(int64_t)s_free[a] * nfree + s_free[b]] = v;
    }
}

}  // namespace

extern "C" {

int pb_lm_residuals(double *residuals_d, const double *bandflux_d, const double *data_d,
                    const double *uncert_d, const int32_t *offset_group_d,
                    const double *offset_vals_d, double offset_unit, int noff,
                    const int32_t *err_group_d, const int32_t *err_mode_d,
                    const double *err_vals_d, double err_unit, int nerr, const double *theta_d,
                    const int32_t *inside_d, const int32_t *gauss_index_d, const double *prior_d,
                    const double *priorlow_d, const double *priorup_d, int ngauss, int nfree,
                    int nwalkers, int ndata, void *stream)
{
    PB_REQUIRE(nwalkers >= 0 && ndata >= 1 && noff >= 0 && nerr >= 0 && ngauss >= 0,
               "pb_lm_residuals: bad shape");
    PB_REQUIRE(nfree >= 1 && nfree <= kMaxParams, "pb_lm_residuals: %d free parameters: 1 to %d",
               nfree, kMaxParams);
    PB_REQUIRE(ngauss <= nfree, "pb_lm_residuals: %d Gaussian priors for %d free parameters",
               ngauss, nfree);
    if (nwalkers == 0)
        return PB_OK;
    PB_REQUIRE(residuals_d && bandflux_d && data_d && uncert_d && inside_d,
               "pb_lm_residuals: null pointer");
    PB_REQUIRE(noff == 0 || (offset_group_d && offset_vals_d),
               "pb_lm_residuals: null pointer (offsets)");
    PB_REQUIRE(nerr == 0 || (err_group_d && err_mode_d && err_vals_d),
               "pb_lm_residuals: null pointer (error models)");
    PB_REQUIRE(ngauss == 0 || (theta_d && gauss_index_d && prior_d && priorlow_d && priorup_d),
               "pb_lm_residuals: null pointer (priors)");
    k_lm_residuals<<<nwalkers, 256, 0, pb::as_stream(stream)>>>(
        residuals_d, bandflux_d, data_d, uncert_d, offset_group_d, offset_vals_d, offset_unit,
        noff, err_group_d, err_mode_d, err_vals_d, err_unit, nerr, theta_d, inside_d,
        gauss_index_d, prior_d, priorlow_d, priorup_d, ngauss, nfree, ndata);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

#define PB_LM_SHAPE(who)                                                                          \
    PB_REQUIRE(nfree >= 1 && nfree <= kMaxParams, who ": %d free parameters: 1 to %d", nfree,     \
               kMaxParams);                                                                       \
    PB_REQUIRE(nstarts >= 0, who ": bad shape")

int pb_lm_probe(double *probe_d, double *step_d, const double *theta_d, const double *pmax_d,
                const double *scale_d, double fd_step, int nfree, int64_t nstarts, void *stream)
{
    PB_LM_SHAPE("pb_lm_probe");
    PB_REQUIRE(fd_step > 0.0 && fd_step < INFINITY, "pb_lm_probe: fd_step must be positive");
    if (nstarts == 0)
        return PB_OK;
    PB_REQUIRE(probe_d && step_d && theta_d && pmax_d && scale_d, "pb_lm_probe: null pointer");
    const int64_t total = nstarts * (nfree + 1) * nfree;
    PB_REQUIRE((total + 255) / 256 <= 0x7fffffffLL, "pb_lm_probe: too many starts");
    k_lm_probe<<<(unsigned)((total + 255) / 256), 256, 0, pb::as_stream(stream)>>>(
        probe_d, step_d, theta_d, pmax_d, scale_d, fd_step, nfree, total);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_lm_normal(double *A_d, double *g_d, double *cost_d, const double *R_d, const double *step_d,
                 int nfree, int m, int64_t nstarts, void *stream)
{
    PB_LM_SHAPE("pb_lm_normal");
    PB_REQUIRE(m >= 1, "pb_lm_normal: m >= 1");
    if (nstarts == 0)
        return PB_OK;
    PB_REQUIRE(A_d && g_d && cost_d && R_d && step_d, "pb_lm_normal: null pointer");
    const int T = (nfree + kTile - 1) / kTile;
    const int ntiles = T * (T + 1) / 2;
    PB_REQUIRE(nstarts * ntiles <= 0x7fffffffLL, "pb_lm_normal: too many starts");
    k_lm_normal<<<(unsigned)(nstarts * ntiles), kNormalBlock, 0, pb::as_stream(stream)>>>(
        A_d, g_d, cost_d, R_d, step_d, nfree, m, ntiles);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int64_t pb_lm_work_doubles(int nfree, int ntrial, int64_t nstarts)
{
    if (nfree < 1 || ntrial < 1 || nstarts < 0)
        return 0;
    const int64_t per = (int64_t)nfree * nfree;
    return nstarts * per * (ntrial > 2 ? ntrial : 2);
}

int pb_lm_step(double *trial_d, double *pgrad_d, double *work_d, const double *A_d,
               const double *g_d, const double *theta_d, const double *lam_d,
               const double *pmin_d, const double *pmax_d, const double *scale_d, double nu,
               int ntrial, int nfree, int64_t nstarts, void *stream)
{
    PB_LM_SHAPE("pb_lm_step");
    PB_REQUIRE(ntrial >= 1 && ntrial <= PB_LM_MAX_TRIALS, "pb_lm_step: %d trials: 1 to %d", ntrial,
               PB_LM_MAX_TRIALS);
    PB_REQUIRE(nu > 1.0 && nu < INFINITY, "pb_lm_step: nu must be above 1");
    if (nstarts == 0)
        return PB_OK;
    PB_REQUIRE(trial_d && pgrad_d && work_d && A_d && g_d && theta_d && lam_d && pmin_d &&
                   pmax_d && scale_d,
               "pb_lm_step: null pointer");
    PB_REQUIRE(nstarts * ntrial <= 0x7fffffffLL, "pb_lm_step: too many starts");
    k_lm_step<<<(unsigned)(nstarts * ntrial), kSolveBlock, 0, pb::as_stream(stream)>>>(
        trial_d, pgrad_d, work_d, A_d, g_d, theta_d, lam_d, pmin_d, pmax_d, scale_d, nu, ntrial,
        nfree);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_lm_update(double *theta_d, double *cost_d, double *lam_d, int32_t *status_d,
                 int32_t *niter_d, int32_t *picked_d, int32_t *unfinished_d,
                 const double *trial_d, const double *Rt_d, const double *pgrad_d,
                 const double *scale_d, double nu, double lam_min, double lam_max, double gtol,
                 double ftol, double xtol, int max_iter, int ntrial, int nfree, int m,
                 int64_t nstarts, void *stream)
{
    PB_LM_SHAPE("pb_lm_update");
    PB_REQUIRE(ntrial >= 1 && ntrial <= PB_LM_MAX_TRIALS, "pb_lm_update: %d trials: 1 to %d",
               ntrial, PB_LM_MAX_TRIALS);
    PB_REQUIRE(m >= 1, "pb_lm_update: m >= 1");
    PB_REQUIRE(nu > 1.0 && nu < INFINITY, "pb_lm_update: nu must be above 1");
    PB_REQUIRE(unfinished_d, "pb_lm_update: null pointer");
    PB_REQUIRE(nstarts <= 0x7fffffffLL, "pb_lm_update: too many starts");
    if (nstarts > 0) {
        PB_REQUIRE(theta_d && cost_d && lam_d && status_d && niter_d && picked_d && trial_d &&
                       Rt_d && pgrad_d && scale_d,
                   "pb_lm_update: null pointer");
        k_lm_update<<<(unsigned)nstarts, 64, 0, pb::as_stream(stream)>>>(
            theta_d, cost_d, lam_d, status_d, niter_d, picked_d, trial_d, Rt_d, pgrad_d, scale_d,
            nu, lam_min, lam_max, gtol, ftol, xtol, max_iter, ntrial, nfree, m);
        PB_LAUNCH_CHECK();
    }
    k_lm_count<<<1, 256, 0, pb::as_stream(stream)>>>(unfinished_d, status_d, nstarts);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_lm_covariance(double *cov_d, int32_t *active_d, int32_t *singular_d, double *work_d,
                     const double *A_d, const double *g_d, const double *theta_d,
                     const double *pmin_d, const double *pmax_d, int nfree, int64_t nstarts,
                     void *stream)
{
    PB_LM_SHAPE("pb_lm_covariance");
    if (nstarts == 0)
        return PB_OK;
    PB_REQUIRE(cov_d && active_d && singular_d && work_d && A_d && g_d && theta_d && pmin_d &&
                   pmax_d,
               "pb_lm_covariance: null pointer");
    PB_REQUIRE(nstarts <= 0x7fffffffLL, "pb_lm_covariance: too many starts");
    k_lm_covariance<<<(unsigned)nstarts, kSolveBlock, 0, pb::as_stream(stream)>>>(
        cov_d, active_d, singular_d, work_d, A_d, g_d, theta_d, pmin_d, pmax_d, nfree);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
