// Partition functions from ExoMol `.states` files (the reference's `pf` step, exomol_states of
// pyratbay/opacity/partitions/partitions.py:389-410: one split() per line in a Python loop, then
// one NumPy pass over all states per temperature).
//
// k_parse_states: one lane parses one record, staged as in pb_linelist.hip (aligned 16-byte loads
// of the workgroup's byte range into LDS), but with 128 records per workgroup, not 256: 17.8 KiB
// of LDS for the 139-byte records of the NH3 lists, so nine workgroups fit a CU and the wavefront
// limit, not LDS, sets the occupancy (profiles/linelist.md names the 41 KiB request and its three
// workgroups per CU as what holds k_parse_hitran back).  The lane reads bytes 0 ... 32 of its
// record with ten dword reads and walks them once in registers: no byte loop over LDS.  The line
// feeds are checked on the way in: the lane that copies a 16-byte block looks for line feeds in
// it and marks the record that has one anywhere but in its last byte.
//
// k_pf_states: Q(T) = sum_j g_j exp(-c2 E_j / T).  Temperatures on the lanes, four per lane, the
// states uniform across the workgroup (their loads are scalar loads).  A workgroup takes one chunk
// of states and one tile of 1024 temperatures and stores one partial per temperature;
// k_pf_reduce adds the partials of a temperature in ascending chunk order.  The argument is
// (-(c2 E_j)) * (1 / T): three roundings (1.5 * 2^-52 * x in the argument), one per state, one per
// temperature, one per term, and no division in the loop.
#include "pb_common.h"
#include "pb_text.h"

namespace {

using namespace pb_text;

constexpr int kRecords = PB_STATES_RECORDS_PER_BLOCK;
constexpr int kScan = 33;                     // bytes 0 ... 32: the tokens end by byte 31
constexpr int kStatesMin = kScan;
constexpr int kIdDigits = 18, kGDigits = 15;  // below 2^63; below 2^53, exact as a double

// an optional '+' and 1 ... maxdig digits (what int() takes beyond that is the host's to read)
struct Unsigned {
    uint64_t v = 0;
    int ndig = 0;
    bool good = true, lead = true;

    __host__ __device__ __forceinline__ void step(uint32_t c, int maxdig)
    {
        const bool plus = lead && c == '+';
        lead = false;
        if (plus)
            return;
        const uint32_t d = c - '0';
        good = good && d < 10u && ndig < maxdig;
        v = v * 10 + (d < 10u ? d : 0);
        ndig += good;
    }
    __host__ __device__ __forceinline__ bool ok() const { return good && ndig > 0; }
};

// One record's bytes 0 ... 32 (f, four to a dword) to its three values and flag bits; fl: the
// layout bit of the line-feed checks.  states_record_host of partitions.py is the same walk in
// Python; __host__ too, so that a host program can run it.
struct StatesFields {
    int64_t id;
    double energy, g;
    uint32_t flags;
};

__host__ __device__ __forceinline__ StatesFields states_fields(
    const uint32_t (&f)[(kScan + 3) / 4], int recsize, uint32_t fl)
{
    Unsigned v_id, v_g;
    Decimal dec;
    int k = 0;                                // index of the token being read, or of the next one
    bool in_token = false;
#pragma unroll
    for (int i = 0; i < kScan; i++) {
        const uint32_t c = (f[i >> 2] >> (8 * (i & 3))) & 0xffu;
        const bool blank = c == ' ' || i == recsize - 1;
        if (blank || (c >= 9 && c <= 13)) {
            if (!blank)
                fl |= PB_LL_STATES_TOKEN;     // split() parts the line there, the layout does not
            if (in_token) {
                if (k == 0 && i > 12)         // the id ends behind byte 11
                    fl |= PB_LL_STATES_LAYOUT;
                k++;
                in_token = false;
            }
        } else {
            if (!in_token) {
                in_token = true;
                if ((k == 1 && i < 12) || (k == 3 && i < 32))
                    fl |= PB_LL_STATES_LAYOUT;
            }
            // a token outside the bytes its layout gives it is flagged above or at its end and
            // its value dropped: the id is read in bytes 0 ... 11 only, the energy in 12 ... 31,
            // the degeneracy in 14 ... 31 (i is a constant of the unrolled loop)
            if (k == 0) {
                if (i < 12)
                    v_id.step(c, kIdDigits);
            } else if (k == 1) {
                if (i >= 12 && i < 32)
                    dec.step(c);
            } else if (k == 2) {
                if (i >= 14 && i < 32)
                    v_g.step(c, kGDigits);
            }
        }
    }
    if (k < 3)                                // a token runs past byte 31, or there are too few
        fl |= in_token ? PB_LL_STATES_LAYOUT : PB_LL_STATES_TOKEN;
    double v_e;
    const bool e_ok = dec.finish(v_e);
    const bool whole = fl & (PB_LL_STATES_TOKEN | PB_LL_STATES_LAYOUT);
    if (!whole) {
        fl |= v_id.ok() ? 0 : PB_LL_STATES_ID;
        fl |= e_ok ? 0 : PB_LL_STATES_ENERGY;
        fl |= v_g.ok() ? 0 : PB_LL_STATES_G;
    }
    StatesFields v;
    v.id = (whole || (fl & PB_LL_STATES_ID)) ? -1 : (int64_t)v_id.v;
    v.energy = (whole || (fl & PB_LL_STATES_ENERGY)) ? __builtin_nan("") : v_e;
    v.g = (whole || (fl & PB_LL_STATES_G)) ? __builtin_nan("") : (double)v_g.v;
    v.flags = fl;
    return v;
}

__global__ __launch_bounds__(kRecords) void k_parse_states(
    const uint8_t *__restrict__ text, int64_t nrec, int recsize, int64_t *__restrict__ id,
    double *__restrict__ energy, double *__restrict__ degeneracy, uint8_t *__restrict__ flags,
    int32_t *nflagged)
{
    extern __shared__ __attribute__((aligned(16))) uint4 s_text[];
    __shared__ uint32_t s_feed[kRecords];     // a line feed before the record's last byte
    const int64_t first = (int64_t)blockIdx.x * kRecords;
    const int n = (int)min((int64_t)kRecords, nrec - first);
    const int t = threadIdx.x;
    s_feed[t] = 0;
    __syncthreads();
    const Staging st = staging(text, first, n, recsize);
    const int nbytes = n * recsize;
    for (int i = t; i < st.nvec; i += kRecords) {
        const uint4 v = st.src[i];
        s_text[i] = v;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t x = w[j] ^ 0x0a0a0a0au;
            if ((x - 0x01010101u) & ~x & 0x80808080u) {       // some byte of x is zero
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int p = 16 * i + 4 * j + b - st.shift;
                    if (((w[j] >> (8 * b)) & 0xffu) == '\n' && p >= 0 && p < nbytes) {
                        const int r = p / recsize;
                        if (p - r * recsize != recsize - 1)
                            s_feed[r] = 1;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (t >= n)
        return;
    const uint32_t *s = (const uint32_t *)s_text;
    const int rec = st.shift + t * recsize;
    uint32_t f[(kScan + 3) / 4];
    field_dwords<kScan>(s, rec, f);
    const int last = rec + recsize - 1;
    const uint32_t c_last = (s[last >> 2] >> (8 * (last & 3))) & 0xffu;
    uint32_t fl = (c_last != '\n' || s_feed[t]) ? PB_LL_STATES_LAYOUT : 0;

    const StatesFields v = states_fields(f, recsize, fl);
    const int64_t r = first + t;
    id[r] = v.id;
    energy[r] = v.energy;
    degeneracy[r] = v.g;
    flags[r] = (uint8_t)v.flags;
    count_flagged(v.flags, nflagged);
}

constexpr int kPfThreads = 256;
constexpr int kPfPerLane = 4;                 // temperatures of a lane: independent exp chains
static_assert(kPfThreads * kPfPerLane == PB_PF_TEMPS_PER_TILE, "tile");

__global__ __launch_bounds__(kPfThreads) void k_pf_states(
    const double *__restrict__ energy, const double *__restrict__ degeneracy, int64_t nstates,
    int chunk, const double *__restrict__ temp, int ntemp, double c2, double *__restrict__ work)
{
    const int tile = blockIdx.y * PB_PF_TEMPS_PER_TILE;
    if (tile + (int)(threadIdx.x & ~63u) >= ntemp)            // a wavefront without a temperature
        return;
    const int64_t j0 = (int64_t)blockIdx.x * chunk;
    const int nj = (int)min((int64_t)chunk, nstates - j0);
    double rt[kPfPerLane], acc[kPfPerLane];
#pragma unroll
    for (int k = 0; k < kPfPerLane; k++) {
        const int t = tile + k * kPfThreads + (int)threadIdx.x;
        rt[k] = t < ntemp ? 1.0 / temp[t] : 0.0;
        acc[k] = 0.0;
    }
    const double *__restrict__ e = energy + j0;
    const double *__restrict__ g = degeneracy + j0;
#pragma unroll 2
    for (int j = 0; j < nj; j++) {
        const double a = -(c2 * e[j]);
        const double gj = g[j];
#pragma unroll
        for (int k = 0; k < kPfPerLane; k++)
            acc[k] = fma(gj, exp(a * rt[k]), acc[k]);
    }
#pragma unroll
    for (int k = 0; k < kPfPerLane; k++) {
        const int t = tile + k * kPfThreads + (int)threadIdx.x;
        if (t < ntemp)
            work[(int64_t)blockIdx.x * ntemp + t] = acc[k];
    }
}

__global__ __launch_bounds__(kPfThreads) void k_pf_reduce(const double *__restrict__ work,
                                                          int nchunks, int ntemp,
                                                          double *__restrict__ q)
{
    const int t = blockIdx.x * kPfThreads + threadIdx.x;
    if (t >= ntemp)
        return;
    double sum = 0.0;
#pragma unroll 8
    for (int c = 0; c < nchunks; c++)
        sum += work[(int64_t)c * ntemp + t];
    q[t] = sum;
}

// the cut of the states: a function of their number alone
void pf_cut(int64_t nstates, int &nchunks, int &chunk)
{
    const int64_t c = (nstates + PB_PF_MAX_CHUNKS - 1) / PB_PF_MAX_CHUNKS;
    chunk = (int)(c < PB_PF_MIN_CHUNK ? PB_PF_MIN_CHUNK : c);
    nchunks = (int)((nstates + chunk - 1) / chunk);
}

}  // namespace

extern "C" {

int pb_parse_states(const uint8_t *text_d, int64_t nrec, int recsize, int64_t *id_d,
                    double *energy_d, double *degeneracy_d, uint8_t *flags_d, int32_t *nflagged_d,
                    void *stream)
{
    PB_REQUIRE(nrec >= 0 && nrec <= INT32_MAX, "pb_parse_states: %lld records: 0 ... 2^31-1",
               (long long)nrec);
    PB_REQUIRE(recsize >= kStatesMin && recsize <= kMaxRecsize,
               "pb_parse_states: records of %d bytes: %d ... %d", recsize, kStatesMin,
               kMaxRecsize);
    if (nrec == 0)                            // nothing to read or write: the pointers may be null
        return PB_OK;
    PB_REQUIRE(text_d && id_d && energy_d && degeneracy_d && flags_d && nflagged_d,
               "pb_parse_states: null pointer");
    k_parse_states<<<pb::div_up(nrec, kRecords), kRecords, lds_bytes(kRecords, recsize),
                     pb::as_stream(stream)>>>(text_d, nrec, recsize, id_d, energy_d,
                                              degeneracy_d, flags_d, nflagged_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_pf_states_work(int64_t nstates, int ntemp, int64_t sizes_h[2])
{
    PB_REQUIRE(nstates >= 0 && nstates <= INT32_MAX, "pb_pf_states: %lld states: 0 ... 2^31-1",
               (long long)nstates);
    PB_REQUIRE(ntemp >= 0 && ntemp <= 65536, "pb_pf_states: %d temperatures: 0 ... 65536", ntemp);
    PB_REQUIRE(sizes_h, "pb_pf_states_work: null pointer");
    int nchunks, chunk;
    pf_cut(nstates, nchunks, chunk);
    sizes_h[0] = (int64_t)nchunks * ntemp;
    sizes_h[1] = chunk;
    return PB_OK;
}

int pb_pf_states(const double *energy_d, const double *degeneracy_d, int64_t nstates,
                 const double *temp_d, int ntemp, double c2, double *q_d, double *work_d,
                 void *stream)
{
    PB_REQUIRE(nstates >= 0 && nstates <= INT32_MAX, "pb_pf_states: %lld states: 0 ... 2^31-1",
               (long long)nstates);
    PB_REQUIRE(ntemp >= 0 && ntemp <= 65536, "pb_pf_states: %d temperatures: 0 ... 65536", ntemp);
    if (ntemp == 0)
        return PB_OK;
    int nchunks, chunk;
    pf_cut(nstates, nchunks, chunk);
    PB_REQUIRE(temp_d && q_d && (nstates == 0 || (energy_d && degeneracy_d && work_d)),
               "pb_pf_states: null pointer");
    if (nchunks > 0) {
        const dim3 grid(nchunks, pb::div_up(ntemp, PB_PF_TEMPS_PER_TILE));
        k_pf_states<<<grid, kPfThreads, 0, pb::as_stream(stream)>>>(
            energy_d, degeneracy_d, nstates, chunk, temp_d, ntemp, c2, work_d);
        PB_LAUNCH_CHECK();
    }
    k_pf_reduce<<<pb::div_up(ntemp, kPfThreads), kPfThreads, 0, pb::as_stream(stream)>>>(
        work_d, nchunks, ntemp, q_d);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // extern "C"
