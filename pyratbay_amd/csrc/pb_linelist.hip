// Line-list ingestion: the text of HITRAN/HITEMP records and of ExoMol transition records to the
// columns of a TLI file (the reference's `runmode = tli`: pyratbay/opacity/linelist/hitran.py:173-203,
// exomol.py:177-204, one seek, one read and five float() calls per record in a Python loop).
//
// One lane parses one record.  A record is 162 bytes (HITRAN with CR LF), 161, or whatever the
// file has, so a lane's record is not dword-aligned in global memory and per-lane byte loads would
// make dozens of sub-dword requests of it.  Instead a workgroup of kBlock lanes copies the
// contiguous byte range of its kBlock records into LDS with aligned 16-byte loads (the start of the
// range rounded down to 16 bytes, the remainder carried as `shift`), and every lane reads its
// record from LDS.
//
// LDS: shift + kBlock * recsize bytes + kSlack, rounded up to 16: 41,504 bytes for 162-byte
// records, so a CU (160 KiB) holds 3 workgroups = 12 wavefronts = 3 per SIMD; 9.5 KiB and the
// wavefront limit (8 per SIMD) for 37-byte ExoMol records.  Registers and scratch (0) of the three
// kernels: profiles/linelist.md.
// Banks: the lane stride is recsize bytes, 40.5 dwords for 162; two lanes are 81 dwords apart,
// which is odd, so the even lanes of a 32-lane group sit on different banks and so do the odd
// ones: a read is 2-way conflicted at worst.  (161: 40.25 dwords, four lanes 161 dwords apart.)
//
// Text to double: the rule of pb_text.h (Decimal).  A field it refuses sets the record's flag bit
// of that field; the host parses those fields itself with float() from the bytes it still holds
// (pyratbay_amd/linelist.py).  The device does not guess.
#include "pb_common.h"
#include "pb_text.h"

namespace {

using namespace pb_text;

constexpr int kBlock = 256;
constexpr int kHitranEnd = 153;               // end of the last field read (g2, [146:153])
constexpr int kExomolMin = 5;                 // "1 2 3"

template <int kLen>
__device__ __forceinline__ bool fixed_field(const uint32_t *s_text, int pos, double &value)
{
    uint32_t f[(kLen + 3) / 4];
    field_dwords<kLen>(s_text, pos, f);
    Decimal dec;
#pragma unroll
    for (int i = 0; i < kLen; i++)
        dec.step((f[i >> 2] >> (8 * (i & 3))) & 0xffu);
    return dec.finish(value);
}

// HITRAN / HITEMP .par records (hitran.py:33-43): isotope character [2], wavenumber [3:15],
// A21 [25:35], Elow [45:55], g2 [146:153]
__global__ __launch_bounds__(kBlock) void k_parse_hitran(
    const uint8_t *__restrict__ text, int64_t nrec, int recsize, double *__restrict__ wn,
    double *__restrict__ elow, double *__restrict__ a21, double *__restrict__ g2,
    int16_t *__restrict__ iso, uint8_t *__restrict__ flags, int32_t *nflagged)
{
    extern __shared__ __attribute__((aligned(16))) uint4 s_text[];
    const int64_t first = (int64_t)blockIdx.x * kBlock;
    const int n = (int)min((int64_t)kBlock, nrec - first);
    const int shift = stage_records<kBlock>(s_text, text, first, n, recsize);
    const int t = threadIdx.x;
    if (t >= n)
        return;
    const uint32_t *s = (const uint32_t *)s_text;
    const int rec = shift + t * recsize;

    // the isotope character and the wavenumber are neighbours: one run of 13 bytes
    uint32_t f[4];
    field_dwords<13>(s, rec + 2, f);
    const uint32_t ic = f[0] & 0xffu;
    // '1'..'9' -> 0..8, '0' -> 9, 'A' -> 10, 'B' -> 11
    const int id = (ic >= '1' && ic <= '9') ? (int)ic - '1'
                   : ic == '0'              ? 9
                   : ic == 'A'              ? 10
                   : ic == 'B'              ? 11
                                            : -1;
    uint32_t fl = id < 0 ? PB_LL_HITRAN_ISO : 0;
    Decimal dec;
#pragma unroll
    for (int i = 1; i < 13; i++)
        dec.step((f[i >> 2] >> (8 * (i & 3))) & 0xffu);
    double v_wn, v_a21, v_elow, v_g2;
    if (!dec.finish(v_wn))
        fl |= PB_LL_HITRAN_WN;
    if (!fixed_field<10>(s, rec + 25, v_a21))
        fl |= PB_LL_HITRAN_A21;
    if (!fixed_field<10>(s, rec + 45, v_elow))
        fl |= PB_LL_HITRAN_ELOW;
    if (!fixed_field<7>(s, rec + 146, v_g2))
        fl |= PB_LL_HITRAN_G2;

    const int64_t r = first + t;
    wn[r] = v_wn;
    elow[r] = v_elow;
    a21[r] = v_a21;
    g2[r] = v_g2;
    iso[r] = (int16_t)id;
    flags[r] = (uint8_t)fl;
    count_flagged(fl, nflagged);
}

// ExoMol .trans records (exomol.py:177-204): the first three tokens are the upper state's id, the
// lower state's id and A21; then wn = E[up] - E[low], elow = E[low], g2 = g[up].
__global__ __launch_bounds__(kBlock) void k_parse_exomol(
    const uint8_t *__restrict__ text, int64_t nrec, int recsize,
    const double *__restrict__ energy, const double *__restrict__ degeneracy, int64_t nstates,
    int isotope, double *__restrict__ wn, double *__restrict__ elow, double *__restrict__ a21,
    double *__restrict__ g2, int16_t *__restrict__ iso, uint8_t *__restrict__ flags,
    int32_t *nflagged)
{
    extern __shared__ __attribute__((aligned(16))) uint4 s_text[];
    const int64_t first = (int64_t)blockIdx.x * kBlock;
    const int n = (int)min((int64_t)kBlock, nrec - first);
    const int shift = stage_records<kBlock>(s_text, text, first, n, recsize);
    const int t = threadIdx.x;
    if (t >= n)
        return;
    const uint8_t *rec = (const uint8_t *)s_text + shift + t * recsize;

    uint32_t fl = 0;
    int p = 0;
    int64_t id[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        while (p < recsize && is_space(rec[p]))
            p++;
        if (p == recsize) {
            fl |= PB_LL_EXOMOL_TOKEN;
            break;
        }
        // an id: an optional '+' and 1 to 18 digits; int() takes more than that (a '-', '_'),
        // which is the host's to read
        int ndig = 0;
        bool good = true;
        uint64_t v = 0;
        if (rec[p] == '+')
            p++;
        for (; p < recsize && !is_space(rec[p]); p++) {
            const uint32_t d = (uint32_t)rec[p] - '0';
            good = good && d < 10u && ndig < 18;
            v = v * 10 + (d < 10u ? d : 0);
            ndig += good;
        }
        if (!(good && ndig > 0))
            fl |= k == 0 ? PB_LL_EXOMOL_UP : PB_LL_EXOMOL_LOW;
        id[k] = (int64_t)v;
    }
    double v_a21 = __builtin_nan("");
    if (!(fl & PB_LL_EXOMOL_TOKEN)) {
        while (p < recsize && is_space(rec[p]))
            p++;
        if (p == recsize) {
            fl |= PB_LL_EXOMOL_TOKEN;
        } else {
            Decimal dec;
            for (; p < recsize && !is_space(rec[p]); p++)
                dec.step(rec[p]);
            if (!dec.finish(v_a21))
                fl |= PB_LL_EXOMOL_A21;
        }
    }
    // an id outside the table is caught here, before any load
    const bool ids = !(fl & (PB_LL_EXOMOL_TOKEN | PB_LL_EXOMOL_UP | PB_LL_EXOMOL_LOW));
    if (ids && !(id[0] >= 0 && id[0] < nstates && id[1] >= 0 && id[1] < nstates))
        fl |= PB_LL_EXOMOL_STATE;
    double v_wn = __builtin_nan(""), v_elow = v_wn, v_g2 = v_wn;
    if (ids && !(fl & PB_LL_EXOMOL_STATE)) {
        const double e_up = energy[id[0]], e_low = energy[id[1]];
        v_wn = e_up - e_low;
        v_elow = e_low;
        v_g2 = degeneracy[id[0]];
    }
    const int64_t r = first + t;
    wn[r] = v_wn;
    elow[r] = v_elow;
    a21[r] = v_a21;
    g2[r] = v_g2;
    iso[r] = (int16_t)isotope;
    flags[r] = (uint8_t)fl;
    count_flagged(fl, nflagged);
}

// gf = g2 * A21 * C1 / (8 pi c) / wn**2 in NumPy's order (hitran.py:199, exomol.py:200): two
// products from the left, a division by the scalar, a division by wn * wn (what NumPy makes of
// `** 2.0`).  The library is built with -ffp-contract=off.
__global__ __launch_bounds__(kBlock) void k_linelist_gf(
    const double *__restrict__ wn, const double *__restrict__ a21, const double *__restrict__ g2,
    int64_t n, double c1, double divisor, double *__restrict__ gf)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        const double w = wn[i];
        gf[i] = g2[i] * a21[i] * c1 / divisor / (w * w);
    }
}

}  // namespace

extern "C" {

int pb_parse_hitran(const uint8_t *text_d, int64_t nrec, int recsize, double *wn_d, double *elow_d,
                    double *a21_d, double *g2_d, int16_t *iso_d, uint8_t *flags_d,
                    int32_t *nflagged_d, void *stream)
{
    PB_REQUIRE(nrec >= 0 && nrec <= INT32_MAX, "pb_parse_hitran: %lld records: 0 ... 2^31-1",
               (long long)nrec);
    PB_REQUIRE(recsize >= kHitranEnd && recsize <= kMaxRecsize,
               "pb_parse_hitran: records of %d bytes: %d (the end of g2) ... %d", recsize,
               kHitranEnd, kMaxRecsize);
    PB_REQUIRE(text_d && wn_d && elow_d && a21_d && g2_d && iso_d && flags_d && nflagged_d,
               "pb_parse_hitran: null pointer");
    if (nrec == 0)
        return PB_OK;
    k_parse_hitran<<<pb::div_up(nrec, kBlock), kBlock, lds_bytes(kBlock, recsize),
                     pb::as_stream(stream)>>>(text_d, nrec, recsize, wn_d, elow_d, a21_d, g2_d,
                                              iso_d, flags_d, nflagged_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_parse_exomol(const uint8_t *text_d, int64_t nrec, int recsize, const double *energy_d,
                    const double *degeneracy_d, int64_t nstates, int iso, double *wn_d,
                    double *elow_d, double *a21_d, double *g2_d, int16_t *iso_d, uint8_t *flags_d,
                    int32_t *nflagged_d, void *stream)
{
    PB_REQUIRE(nrec >= 0 && nrec <= INT32_MAX, "pb_parse_exomol: %lld records: 0 ... 2^31-1",
               (long long)nrec);
    PB_REQUIRE(recsize >= kExomolMin && recsize <= kMaxRecsize,
               "pb_parse_exomol: records of %d bytes: %d ... %d", recsize, kExomolMin,
               kMaxRecsize);
    PB_REQUIRE(nstates >= 1, "pb_parse_exomol: %lld states: at least 1", (long long)nstates);
    PB_REQUIRE(iso >= 0 && iso <= INT16_MAX, "pb_parse_exomol: isotope index %d: 0 ... 32767",
               iso);
    PB_REQUIRE(text_d && energy_d && degeneracy_d && wn_d && elow_d && a21_d && g2_d && iso_d &&
                   flags_d && nflagged_d,
               "pb_parse_exomol: null pointer");
    if (nrec == 0)
        return PB_OK;
    k_parse_exomol<<<pb::div_up(nrec, kBlock), kBlock, lds_bytes(kBlock, recsize),
                     pb::as_stream(stream)>>>(text_d, nrec, recsize, energy_d, degeneracy_d,
                                              nstates, iso, wn_d, elow_d, a21_d, g2_d, iso_d,
                                              flags_d, nflagged_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_linelist_gf(const double *wn_d, const double *a21_d, const double *g2_d, int64_t n,
                   double c1, double divisor, double *gf_d, void *stream)
{
    PB_REQUIRE(n >= 0 && n <= INT32_MAX, "pb_linelist_gf: %lld lines: 0 ... 2^31-1",
               (long long)n);
    PB_REQUIRE(wn_d && a21_d && g2_d && gf_d, "pb_linelist_gf: null pointer");
    if (n == 0)
        return PB_OK;
    k_linelist_gf<<<pb::div_up(n, kBlock), kBlock, 0, pb::as_stream(stream)>>>(
        wn_d, a21_d, g2_d, n, c1, divisor, gf_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
