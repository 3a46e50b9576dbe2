// Co-add grouping of a line list on the device (the static pre-pass of pb_lines_create).
//
// Reference: the sequential loop of _extcoeff.extinction, src_c/_extcoeff.c:230-262 -- for every
// in-range line in file order: nearest fine-grid index iown (:243-245), then the FOLLOWING lines
// of the same isotope with lwn <= own[last] and |lwn - own[iown]| < ownstep are co-added to it
// (:248-262) and skipped.  Which lines lead a group depends only on (lwn, lID, own): it is done
// once per line list.
//
// The greedy scan is a chain (the line after a group's last member leads the next group), made
// parallel with forward pointers:
//   k_classify   per line: in range?, iown, the fine-grid wavenumber it snaps to
//   k_next       per line: the end of the group it WOULD lead (bisection on the sorted wavenumbers
//                of its isotope) and nxt = the next in-range line at or after that end
//   k_block_exit per block of 1024 lines: pointer doubling inside the block -> for every line the
//                first line of its chain that lies beyond the block
//   k_chain      one thread: from the first in-range line, block to block through the exits
//                (n/1024 dependent steps), noting where the chain enters every block
//   k_mark       one thread per block: follows nxt from the block's entry and marks the leaders
//   scan + k_emit: leaders compacted in file order = (isotope, position) order.
// Requires the TLI invariant: lines sorted by isotope, then wavenumber (checked on the device;
// otherwise the host loop of pb_lines_create does the work).
//
// Also of the TLI stage: the partition functions of a database's isotopes at the temperatures of a
// batch of atmospheres (k_iso_partition, pb_iso_partition).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <vector>

#include "pb_common.h"
#include "pb_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kChainBlock = 1024;

struct GridDesc {
    const double *own;       // fine grid on the device, or null: own0 + i*step
    double own0, lo, hi, step;
    int64_t onwn;
};

__device__ inline double own_at(const GridDesc &g, int64_t i)
{
    if (g.own)
        return g.own[i];
    const double prod = __dmul_rn((double)i, g.step);       // multiply, then add, like NumPy
    return __dadd_rn(g.own0, prod);
}

__global__ __launch_bounds__(kBlock) void k_check_sorted(int *bad, const double *lwn,
                                                         const int32_t *lid, int64_t n)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j == 0 || j >= n)
        return;
    if (lid[j] < lid[j - 1] || (lid[j] == lid[j - 1] && lwn[j] < lwn[j - 1]))
        *bad = 1;
}

__global__ __launch_bounds__(kBlock) void k_classify(int32_t *iown_out, double *centre_out,
                                                     const double *lwn, GridDesc g, int64_t n)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n)
        return;
    const double v = lwn[j];
    if (v < g.lo || v > g.hi) {
        iown_out[j] = -1;
        centre_out[j] = 0.0;
        return;
    }
    int64_t iown = (int64_t)((v - g.lo) / g.step);
    if (iown + 1 < g.onwn && fabs(v - own_at(g, iown + 1)) < fabs(v - own_at(g, iown)))
        iown++;
    iown_out[j] = (int32_t)iown;
    centre_out[j] = own_at(g, iown);
}

// end[j]: first line after j that is NOT co-added to a group led by j; nxt[j]: the next group
// leader if j leads one (first in-range line at or after end[j]).  iso_lend[s] = one past the
// last line of isotope s, iso_next_first[s] = first in-range line of the isotopes after s.
__global__ __launch_bounds__(kBlock) void k_next(int32_t *end_out, int32_t *nxt_out,
                                                 const double *lwn, const int32_t *lid,
                                                 const int32_t *iown, const double *centre,
                                                 const int64_t *iso_lend,
                                                 const int64_t *iso_next_first, GridDesc g,
                                                 int64_t n)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n)
        return;
    const int s = lid[j];
    const int64_t send = iso_lend[s];
    if (iown[j] < 0) {
        // not a leader candidate: only a stepping stone for the pointer doubling
        end_out[j] = (int32_t)(j + 1);
        int64_t k = j + 1;
        if (k >= send || lwn[j] > g.hi)
            k = iso_next_first[s];
        // lines below the range precede the in-range ones of their isotope
        nxt_out[j] = (int32_t)min(k, n);
        return;
    }
    const double c = centre[j];
    int64_t lo = j + 1, hi = send;                // first k in (j, send) failing the predicate
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const double v = lwn[mid];
        if (v <= g.hi && fabs(v - c) < g.step)
            lo = mid + 1;
        else
            hi = mid;
    }
    end_out[j] = (int32_t)lo;
    int64_t k = lo;
    if (k >= send || lwn[k] > g.hi)
        k = iso_next_first[s];
    nxt_out[j] = (int32_t)min(k, n);
}

// lines of an isotope that lie below the range point to ... the next line; fix them up so that a
// chain entering there reaches the first in-range line (only the pointer doubling walks them)
__global__ __launch_bounds__(kChainBlock) void k_block_exit(int32_t *exit_out, const int32_t *nxt,
                                                            int64_t n)
{
    __shared__ int32_t s_e[2][kChainBlock];
    const int64_t base = (int64_t)blockIdx.x * kChainBlock;
    const int t = threadIdx.x;
    const int64_t j = base + t;
    const int64_t bend = base + kChainBlock;
    int32_t e = j < n ? nxt[j] : (int32_t)n;
    int cur = 0;
    s_e[0][t] = e;
    __syncthreads();
    for (int round = 0; round < 10; round++) {
        if (e < bend && e < n)
            e = s_e[cur][e - base];
        s_e[cur ^ 1][t] = e;
        cur ^= 1;
        __syncthreads();
    }
    if (j < n)
        exit_out[j] = e;
}

__global__ void k_chain(int32_t *entry, const int32_t *exit_ptr, int64_t first, int64_t n)
{
    int64_t e = first;
    while (e < n) {
        entry[e / kChainBlock] = (int32_t)e;
        e = exit_ptr[e];
    }
}

__global__ __launch_bounds__(kBlock) void k_mark(int32_t *leader, const int32_t *entry,
                                                 const int32_t *nxt, int64_t n, int nblocks)
{
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= nblocks)
        return;
    const int64_t bend = min((int64_t)(b + 1) * kChainBlock, n);
    int64_t j = entry[b];
    while (j >= 0 && j < bend) {
        leader[j] = 1;
        j = nxt[j];
    }
}

__global__ __launch_bounds__(kBlock) void k_emit(int32_t *gfirst, int32_t *gcount, int32_t *giown,
                                                 int32_t *giso, const int32_t *leader,
                                                 const int32_t *gpos, const int32_t *end_ptr,
                                                 const int32_t *iown, const int32_t *lid,
                                                 int64_t n)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n || !leader[j])
        return;
    const int g = gpos[j];
    gfirst[g] = (int32_t)j;
    gcount[g] = end_ptr[j] - (int32_t)j;
    giown[g] = iown[j];
    giso[g] = lid[j];
}

// ---------------------------------------------------------------------------
// Partition functions Z_i(T) of the isotopes of one TLI database at the layer temperatures of a
// batch of atmospheres (line_by_line.py:156-158: interp1d(db.temp, db.iso_pf[j], kind='slinear');
// :219-222: evaluated at the temperature profile on every extinction call).  SciPy's first-order
// spline is evaluated as its de Boor recurrence does (w = 1/(t_hi - t_lo); Z = z_lo (w (t_hi - T))
// + z_hi (w (T - t_lo)), interval t_lo <= T < t_hi, the last one closed): bit-equal to it.  A
// temperature outside the table is an error in the reference (interp1d raises): NaN is written
// and counted in *nbad.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_iso_partition(
    double *z, int64_t z_iso_stride, int64_t z_t_stride, const double *temp, int64_t ntemp,
    const double *ttab, int ntab, const double *pf, int niso, int32_t *nbad)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= ntemp)
        return;
    const double x = temp[t];
    if (!(x >= ttab[0] && x <= ttab[ntab - 1])) {
        for (int i = 0; i < niso; i++)
            z[i * z_iso_stride + t * z_t_stride] = __longlong_as_double(0x7ff8000000000000ll);
        if (nbad)
            atomicAdd(nbad, 1);
        return;
    }
    int lo = 0, hi = ntab - 1;                 // largest lo <= ntab - 2 with ttab[lo] <= x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ttab[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    const double xa = ttab[lo], xb = ttab[lo + 1];
    const double w = 1.0 / (xb - xa);
    const double h0 = w * (xb - x), h1 = w * (x - xa);
    for (int i = 0; i < niso; i++) {
        const double *row = pf + (int64_t)i * ntab;
        z[i * z_iso_stride + t * z_t_stride] = row[lo] * h0 + row[lo + 1] * h1;
    }
}

template <typename T>
struct DevBuf {
    T *p = nullptr;
    ~DevBuf() { (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)); }
};

}  // namespace

// Groups of the line list already on the device (l->d_lwn, l->d_lid); fills l->d_gfirst,
// d_gcount, d_giown, d_giso, the host mirrors, iso_gstart, ngroups, nadd, ninrange.
// Returns PB_OK, an error, or 1 when the list is not sorted by (isotope, wavenumber): the caller
// then runs the host loop.
int pb_lines_group_device(pb_lines *l, const double *lwn_h, const int32_t *lid_h,
                          const double *own_h)
{
    const int64_t n = l->nlines;
    const int niso = l->niso;
    if (n == 0)
        return 1;
    hipStream_t s = nullptr;
    DevBuf<int> bad;
    PB_HIP(bad.alloc(1));
    PB_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), s));
    const unsigned nb = (unsigned)pb::div_up(n, kBlock);
    k_check_sorted<<<nb, kBlock, 0, s>>>(bad.p, l->d_lwn, l->d_lid, n);
    PB_LAUNCH_CHECK();
    int unsorted = 0;
    PB_HIP(hipMemcpy(&unsorted, bad.p, sizeof(int), hipMemcpyDeviceToHost));
    if (unsorted)
        return 1;

    // per isotope: its line segment and the first in-range line of the isotopes after it
    // (bisections over the sorted host arrays)
    std::vector<int64_t> lend((size_t)niso, 0), next_first((size_t)niso, n);
    std::vector<int64_t> first_in((size_t)niso, -1);
    {
        int64_t at = 0;
        for (int i = 0; i < niso; i++) {
            const int32_t *e = std::upper_bound(lid_h + at, lid_h + n, (int32_t)i);
            const int64_t b0 = at, b1 = e - lid_h;
            lend[(size_t)i] = b1;
            const double *f = std::lower_bound(lwn_h + b0, lwn_h + b1, l->own0);
            if (f != lwn_h + b1 && *f <= l->own_last)
                first_in[(size_t)i] = f - lwn_h;
            at = b1;
        }
        int64_t nf = n;
        for (int i = niso - 1; i >= 0; i--) {
            next_first[(size_t)i] = nf;
            if (first_in[(size_t)i] >= 0)
                nf = first_in[(size_t)i];
        }
        // nf = first in-range line of the whole list
        l->iso_gstart.assign((size_t)niso + 1, 0);
        if (nf >= n) {                                   // nothing in range
            l->ngroups = 0;
            l->h_gfirst.clear();
            l->h_gcount.clear();
            l->h_giown.clear();
            PB_HIP(hipMalloc(&l->d_gfirst, 4));
            PB_HIP(hipMalloc(&l->d_gcount, 4));
            PB_HIP(hipMalloc(&l->d_giown, 4));
            PB_HIP(hipMalloc(&l->d_giso, 4));
            return PB_OK;
        }
        first_in.push_back(nf);
    }
    const int64_t first = first_in.back();

    GridDesc g;
    DevBuf<double> own_d;
    g.own = nullptr;
    if (own_h) {
        PB_HIP(own_d.alloc((size_t)l->onwn));
        PB_HIP(hipMemcpy(own_d.p, own_h, (size_t)l->onwn * 8, hipMemcpyHostToDevice));
        g.own = own_d.p;
    }
    g.own0 = l->own0;
    g.lo = l->own0;
    g.hi = l->own_last;
    g.step = l->ownstep;
    g.onwn = l->onwn;

    DevBuf<int32_t> iown, endp, nxt, exitp, entry, leader, gpos;
    DevBuf<double> centre;
    DevBuf<int64_t> lend_d, nf_d;
    const int nblocks = pb::div_up(n, kChainBlock);
    PB_HIP(iown.alloc((size_t)n));
    PB_HIP(centre.alloc((size_t)n));
    PB_HIP(endp.alloc((size_t)n));
    PB_HIP(nxt.alloc((size_t)n));
    PB_HIP(exitp.alloc((size_t)n));
    PB_HIP(entry.alloc((size_t)nblocks));
    PB_HIP(leader.alloc((size_t)n));
    PB_HIP(gpos.alloc((size_t)n + 1));
    PB_HIP(lend_d.alloc((size_t)niso));
    PB_HIP(nf_d.alloc((size_t)niso));
    PB_HIP(hipMemcpy(lend_d.p, lend.data(), (size_t)niso * 8, hipMemcpyHostToDevice));
    PB_HIP(hipMemcpy(nf_d.p, next_first.data(), (size_t)niso * 8, hipMemcpyHostToDevice));
    PB_HIP(hipMemsetAsync(entry.p, 0xff, (size_t)nblocks * 4, s));
    PB_HIP(hipMemsetAsync(leader.p, 0, (size_t)n * 4, s));

    k_classify<<<nb, kBlock, 0, s>>>(iown.p, centre.p, l->d_lwn, g, n);
    PB_LAUNCH_CHECK();
    k_next<<<nb, kBlock, 0, s>>>(endp.p, nxt.p, l->d_lwn, l->d_lid, iown.p, centre.p, lend_d.p,
                                 nf_d.p, g, n);
    PB_LAUNCH_CHECK();
    k_block_exit<<<nblocks, kChainBlock, 0, s>>>(exitp.p, nxt.p, n);
    PB_LAUNCH_CHECK();
    k_chain<<<1, 1, 0, s>>>(entry.p, exitp.p, first, n);
    PB_LAUNCH_CHECK();
    k_mark<<<pb::div_up(nblocks, kBlock), kBlock, 0, s>>>(leader.p, entry.p, nxt.p, n, nblocks);
    PB_LAUNCH_CHECK();
    // exclusive scan of the leader flags -> position of every group
    {
        size_t tb = 0;
        PB_HIP(rocprim::exclusive_scan(nullptr, tb, leader.p, gpos.p, 0, (size_t)n,
                                       rocprim::plus<int32_t>(), s));
        DevBuf<unsigned char> tmp;
        PB_HIP(tmp.alloc(tb));
        PB_HIP(rocprim::exclusive_scan(tmp.p, tb, leader.p, gpos.p, 0, (size_t)n,
                                       rocprim::plus<int32_t>(), s));
        PB_HIP(hipStreamSynchronize(s));
    }
    int32_t last_pos = 0, last_flag = 0;
    PB_HIP(hipMemcpy(&last_pos, gpos.p + (n - 1), 4, hipMemcpyDeviceToHost));
    PB_HIP(hipMemcpy(&last_flag, leader.p + (n - 1), 4, hipMemcpyDeviceToHost));
    const int64_t ng = (int64_t)last_pos + last_flag;
    l->ngroups = ng;
    PB_HIP(hipMalloc(&l->d_gfirst, std::max<int64_t>(ng, 1) * 4));
    PB_HIP(hipMalloc(&l->d_gcount, std::max<int64_t>(ng, 1) * 4));
    PB_HIP(hipMalloc(&l->d_giown, std::max<int64_t>(ng, 1) * 4));
    PB_HIP(hipMalloc(&l->d_giso, std::max<int64_t>(ng, 1) * 4));
    k_emit<<<nb, kBlock, 0, s>>>(l->d_gfirst, l->d_gcount, l->d_giown, l->d_giso, leader.p,
                                 gpos.p, endp.p, iown.p, l->d_lid, n);
    PB_LAUNCH_CHECK();
    l->h_gfirst.resize((size_t)ng);
    l->h_gcount.resize((size_t)ng);
    l->h_giown.resize((size_t)ng);
    PB_HIP(hipMemcpy(l->h_gfirst.data(), l->d_gfirst, (size_t)ng * 4, hipMemcpyDeviceToHost));
    PB_HIP(hipMemcpy(l->h_gcount.data(), l->d_gcount, (size_t)ng * 4, hipMemcpyDeviceToHost));
    PB_HIP(hipMemcpy(l->h_giown.data(), l->d_giown, (size_t)ng * 4, hipMemcpyDeviceToHost));
    // per-isotope group segments: groups before the first line of each isotope
    for (int i = 0; i <= niso; i++) {
        const int64_t line = i == 0 ? 0 : lend[(size_t)i - 1];
        int32_t v = (int32_t)ng;
        if (line < n)
            PB_HIP(hipMemcpy(&v, gpos.p + line, 4, hipMemcpyDeviceToHost));
        l->iso_gstart[(size_t)i] = v;
    }
    int64_t members = 0;
    for (int32_t c : l->h_gcount)
        members += c;
    l->ninrange = members;
    l->nadd = members - ng;
    return PB_OK;
}

extern "C" {

// ---------------------------------------------------------------------------
// line list: the C ABI
// ---------------------------------------------------------------------------
int pb_lines_create(pb_lines **out, const double *lwn_h, const double *elow_h,
                    const double *gf_h, const int32_t *lid_h, int64_t nlines, int niso,
                    const double *own_h, int64_t onwn, double own0, double ownstep)
{
    PB_REQUIRE(out, "pb_lines_create: null out");
    *out = nullptr;
    PB_REQUIRE(nlines >= 0 && niso > 0 && onwn >= 2, "pb_lines_create: bad sizes");
    PB_REQUIRE(nlines == 0 || (lwn_h && elow_h && gf_h && lid_h),
               "pb_lines_create: null line arrays");
    PB_REQUIRE(nlines < 2147483647LL && onwn < 2147483647LL,
               "pb_lines_create: sizes exceed the reference's 32-bit indices");
    // own[] generated exactly like NumPy (wnlow + arange*ownstep: multiply, then add)
    auto own_at = [&](int64_t i) -> double {
        if (own_h)
            return own_h[i];
        volatile double prod = (double)i * ownstep;
        return own0 + prod;
    };
    pb_lines *l = new (std::nothrow) pb_lines();
    if (!l)
        return PB_ERR_NOMEM;
    l->nlines = nlines;
    l->niso = niso;
    l->onwn = onwn;
    l->own0 = own_at(0);
    l->own_last = own_at(onwn - 1);
    l->ownstep = own_at(1) - own_at(0);
    const double lo = l->own0, hi = l->own_last, step = l->ownstep;

    l->h_lwn.assign(lwn_h, lwn_h + nlines);
    l->h_elow.assign(elow_h, elow_h + nlines);
    l->h_gf.assign(gf_h, gf_h + nlines);
    int rc = PB_OK;
    if (rc == PB_OK) rc = pb::upload(&l->d_lwn, lwn_h, (size_t)nlines);
    if (rc == PB_OK) rc = pb::upload(&l->d_elow, elow_h, (size_t)nlines);
    if (rc == PB_OK) rc = pb::upload(&l->d_gf, gf_h, (size_t)nlines);
    if (rc == PB_OK) rc = pb::upload(&l->d_lid, lid_h, (size_t)nlines);
    if (rc != PB_OK) {
        pb_lines_destroy(l);
        return rc;
    }
    // Grouping on the device (pb_lines.hip) when the list has the TLI order (isotope, then
    // wavenumber) and valid isotope ids; PB_LINES_HOST=1 or any other order: the host loop below
    bool grouped = false;
    if (nlines > 0 && !getenv("PB_LINES_HOST") && lid_h[0] >= 0 && lid_h[nlines - 1] < niso) {
        const int grc = pb_lines_group_device(l, lwn_h, lid_h, own_h);
        if (grc == PB_OK) {
            grouped = true;
            l->grouped_on_device = 1;
        } else if (grc != 1) {
            pb_lines_destroy(l);
            return grc;
        }
    }
    if (!grouped) {
    struct Group {
        int32_t first, count, iown, iso;
    };
    std::vector<Group> groups;
    groups.reserve((size_t)nlines);
    // The lines of ONE isotope must come in ascending wavenumber order (isotopes may interleave).
    // The reference's Doppler-width index is a one-way search from the isotope's previous line
    // (_extcoeff.c:278, utils.h:45-72: `if (value < array[lo]) return lo`): on a list that steps
    // back within an isotope it keeps a stale index, a result that depends on the list order and
    // on which lines the layer's threshold skipped.  The kernels evaluate the nearest index
    // statelessly -- the same thing on an ordered list, NOT on such a one: refuse it loudly.
    // (Every TLI reader output is ordered; the reference itself produces an unordered list only
    // from a TLI FILE holding several databases, whose isotope ids it confuses:
    // line_by_line.py:114-119, fixture G16 `onefile`.)
    std::vector<double> last_wn((size_t)niso, -HUGE_VAL);
    for (int64_t ln = 0; ln < nlines; ln++) {
        const int i = lid_h[ln];
        if (i < 0 || i >= niso) {
            pb::set_error("pb_lines_create: line %lld has isotope id %d outside [0,%d)",
                          (long long)ln, i, niso);
            pb_lines_destroy(l);
            return PB_ERR_ARG;
        }
        const double v = lwn_h[ln];
        if (v < lo || v > hi)
            continue;
        if (v < last_wn[(size_t)i]) {
            pb::set_error("pb_lines_create: line %lld (%.6f cm-1) of isotope %d comes after a "
                          "line at %.6f cm-1: the lines of an isotope must be in ascending "
                          "wavenumber order (the reference's Doppler-index search is one-way, "
                          "_extcoeff.c:278; its result on such a list is order-dependent)",
                          (long long)ln, v, i, last_wn[(size_t)i]);
            pb_lines_destroy(l);
            return PB_ERR_ARG;
        }
        last_wn[(size_t)i] = v;
        l->ninrange++;
        // nearest fine-grid index (_extcoeff.c:243-245)
        int64_t iown = (int64_t)((v - lo) / step);
        if (iown + 1 < onwn && fabs(v - own_at(iown + 1)) < fabs(v - own_at(iown)))
            iown++;
        Group g{(int32_t)ln, 1, (int32_t)iown, i};
        const double centre = own_at(iown);
        // greedy co-adding of the following lines of the same isotope (:248-262)
        while (ln + 1 != nlines && lid_h[ln + 1] == i && lwn_h[ln + 1] <= hi) {
            if (fabs(lwn_h[ln + 1] - centre) < step) {
                ln++;
                last_wn[(size_t)i] = std::max(last_wn[(size_t)i], lwn_h[ln]);
                g.count++;
                l->nadd++;
                l->ninrange++;
            } else
                break;
        }
        groups.push_back(g);
    }
    // (isotope, fine index) order; stable, so a sorted TLI keeps its file order
    std::stable_sort(groups.begin(), groups.end(), [](const Group &x, const Group &y) {
        return x.iso != y.iso ? x.iso < y.iso : x.iown < y.iown;
    });
    l->ngroups = (int64_t)groups.size();
    l->iso_gstart.assign((size_t)niso + 1, 0);
    for (const Group &g : groups)
        l->iso_gstart[(size_t)g.iso + 1]++;
    for (int i = 0; i < niso; i++)
        l->iso_gstart[(size_t)i + 1] += l->iso_gstart[(size_t)i];
    std::vector<int32_t> &gfirst = l->h_gfirst, &gcount = l->h_gcount, &giown = l->h_giown;
    gfirst.resize(groups.size());
    gcount.resize(groups.size());
    giown.resize(groups.size());
    std::vector<int32_t> giso(groups.size());
    for (size_t k = 0; k < groups.size(); k++) {
        gfirst[k] = groups[k].first;
        gcount[k] = groups[k].count;
        giown[k] = groups[k].iown;
        giso[k] = groups[k].iso;
    }
    if (rc == PB_OK) rc = pb::upload(&l->d_gfirst, gfirst.data(), gfirst.size());
    if (rc == PB_OK) rc = pb::upload(&l->d_gcount, gcount.data(), gcount.size());
    if (rc == PB_OK) rc = pb::upload(&l->d_giown, giown.data(), giown.size());
    if (rc == PB_OK) rc = pb::upload(&l->d_giso, giso.data(), giso.size());
    }
    if (rc == PB_OK) rc = pb::upload(&l->d_iso_gstart, l->iso_gstart.data(), l->iso_gstart.size());
    if (rc != PB_OK) {
        pb_lines_destroy(l);
        return rc;
    }
    *out = l;
    return PB_OK;
}

int pb_lines_grouped_on_device(const pb_lines *l, int *flag)
{
    PB_REQUIRE(l && flag, "pb_lines_grouped_on_device: null pointer");
    *flag = l->grouped_on_device;
    return PB_OK;
}

int pb_lines_groups(const pb_lines *l, int32_t *first_h, int32_t *count_h, int32_t *iown_h,
                    int64_t *iso_gstart_h)
{
    PB_REQUIRE(l, "pb_lines_groups: null handle");
    const size_t n = (size_t)l->ngroups;
    if (first_h)
        std::copy(l->h_gfirst.begin(), l->h_gfirst.begin() + n, first_h);
    if (count_h)
        std::copy(l->h_gcount.begin(), l->h_gcount.begin() + n, count_h);
    if (iown_h)
        std::copy(l->h_giown.begin(), l->h_giown.begin() + n, iown_h);
    if (iso_gstart_h)
        std::copy(l->iso_gstart.begin(), l->iso_gstart.end(), iso_gstart_h);
    return PB_OK;
}

int pb_lines_stats(const pb_lines *l, int64_t stats[3])
{
    PB_REQUIRE(l && stats, "pb_lines_stats: null pointer");
    stats[0] = l->ninrange;
    stats[1] = l->ngroups;
    stats[2] = l->nadd;
    return PB_OK;
}

int pb_iso_partition(double *z_d, int64_t z_iso_stride, int64_t z_t_stride,
                     const double *temp_d, int64_t ntemp, const double *ttab_d, int ntab,
                     const double *pf_d, int niso, int32_t *nbad_d, void *stream)
{
    PB_REQUIRE(ntemp >= 0 && niso >= 0 && ntab >= 2, "pb_iso_partition: bad shape (a partition-"
               "function table needs at least two temperatures, got %d)", ntab);
    if (ntemp == 0 || niso == 0)
        return PB_OK;
    PB_REQUIRE(z_d && temp_d && ttab_d && pf_d, "pb_iso_partition: null pointer");
    k_iso_partition<<<(unsigned)pb::div_up(ntemp, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        z_d, z_iso_stride, z_t_stride, temp_d, ntemp, ttab_d, ntab, pf_d, niso, nbad_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

void pb_lines_destroy(pb_lines *l)
{
    if (!l)
        return;
    (void)hipFree(l->d_lwn);
    (void)hipFree(l->d_elow);
    (void)hipFree(l->d_gf);
    (void)hipFree(l->d_lid);
    (void)hipFree(l->d_gfirst);
    (void)hipFree(l->d_gcount);
    (void)hipFree(l->d_giown);
    (void)hipFree(l->d_giso);
    (void)hipFree(l->d_iso_gstart);
    delete l;
}

}  // extern "C"
