// Text records to numbers: what the line-list kernels (pb_linelist.hip) and the states kernel
// (pb_partitions.hip) share.  The staging of a workgroup's records into LDS, the dword reads of a
// field, and the one rule by which a decimal field becomes a double.
//
// Text to double.  A field is blanks, a sign, digits with at most one point, an exponent, blanks.
// It gives an integer w of its digits and a decimal exponent q.  If w <= 2^53 and |q| <= 22 the
// value is double(w) * 1e q or double(w) / 1e -q: both operands are exact, so the one IEEE
// operation rounds correctly and returns the bits of Python's float() (Clinger's fast path).
// Every other field -- more digits, a larger exponent, nan, inf, an underscore, an empty field,
// any byte outside this grammar -- is refused; the host parses those fields itself with float()
// from the bytes it still holds (pyratbay_amd/linelist.py).  The device does not guess.
#pragma once
#include "pb_common.h"

namespace pb_text {

constexpr int kMaxRecsize = 255;              // shift + 256 * 255 + slack stays within 64 KiB
constexpr int kSlack = 16;                    // dword reads of a field's last bytes end inside it

// 1e0 ... 1e22: the powers of ten a double holds exactly
__host__ __device__ __forceinline__ double pow10_exact(int q)
{
    constexpr double table[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,
                                  1e8,  1e9,  1e10, 1e11, 1e12, 1e13, 1e14, 1e15,
                                  1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    return table[q];
}

// The field grammar as a machine fed one byte at a time (decimal_fast_path_host of linelist.py is
// the same machine in Python; __host__ too, so that a host program can run it against strtod).
struct Decimal {
    enum { LEAD, SIGN, INT, FRAC, EXP, EXPSIGN, EXPDIG, TRAIL, BAD };
    uint64_t w = 0;          // the digits, leading zeros dropped, at most 19 of them
    int nsig = 0;            // digits from the first non-zero one on
    int ndig = 0;            // digits of the mantissa
    int nfrac = 0;           // of them behind the point
    int ex = 0;              // exponent digits (clamped: anything above 22 is flagged anyway)
    int state = LEAD;
    bool neg = false, eneg = false;

    __host__ __device__ __forceinline__ void step(uint32_t c)
    {
        const uint32_t d = c - '0';
        if (d < 10u) {
            if (state <= FRAC) {
                if (state < INT)
                    state = INT;
                ndig++;
                nfrac += state == FRAC;
                nsig += (w != 0 || d != 0);
                if (nsig <= 19)
                    w = w * 10 + d;
            } else if (state <= EXPDIG) {
                state = EXPDIG;
                ex = ex * 10 + (int)d;
                ex = ex > 100000 ? 100000 : ex;
            } else {
                state = BAD;
            }
        } else if (c == ' ') {
            if (state == INT || state == FRAC || state == EXPDIG)
                state = TRAIL;
            else if (state != LEAD && state != TRAIL)
                state = BAD;
        } else if (c == '.') {
            state = state <= INT ? FRAC : BAD;
        } else if (c == 'e' || c == 'E') {
            state = ((state == INT || state == FRAC) && ndig > 0) ? EXP : BAD;
        } else if (c == '+' || c == '-') {
            if (state == LEAD) {
                state = SIGN;
                neg = c == '-';
            } else if (state == EXP) {
                state = EXPSIGN;
                eneg = c == '-';
            } else {
                state = BAD;
            }
        } else {
            state = BAD;
        }
    }

    // the value when the field is on the fast path; false: the host parses it
    __host__ __device__ __forceinline__ bool finish(double &value) const
    {
        const bool grammar = ndig > 0 &&
                             (state == INT || state == FRAC || state == EXPDIG || state == TRAIL);
        const int q = (eneg ? -ex : ex) - nfrac;
        if (!(grammar && nsig <= 19 && w <= (1ull << 53) && q >= -22 && q <= 22)) {
            value = __builtin_nan("");
            return false;
        }
        const double m = (double)w;                          // exact: w <= 2^53
        const double v = q < 0 ? m / pow10_exact(-q) : m * pow10_exact(q);
        value = neg ? -v : v;
        return true;
    }
};

// kLen bytes of LDS from byte position `pos` on, as aligned dword reads shifted into place: out[j]
// holds bytes 4j .. 4j+3 of the field (ds_read_b32 of an unaligned address is not an option, and
// one ds_read_u8 per character is 2.5 times as many LDS instructions)
template <int kLen>
__device__ __forceinline__ void field_dwords(const uint32_t *s_text, int pos,
                                             uint32_t (&out)[(kLen + 3) / 4])
{
    constexpr int n = (kLen + 3) / 4;
    const uint32_t *p = s_text + (pos >> 2);
    const uint32_t sh = pos & 3;
    uint32_t d[n + 1];
#pragma unroll
    for (int j = 0; j <= n; j++)
        d[j] = p[j];
#pragma unroll
    for (int j = 0; j < n; j++)
        out[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
}

// The range of 16-byte blocks that hold at least one byte of records first .. first + nrec - 1
// (such a block lies in the same page as that byte, so the bytes of it before the first record or
// after the last one are readable; they are not used): its first block, how far the first record
// lies behind the block's start, and the number of blocks.
struct Staging {
    const uint4 *src;
    int shift, nvec;
};

__device__ __forceinline__ Staging staging(const uint8_t *text, int64_t first, int nrec,
                                           int recsize)
{
    const uintptr_t start = (uintptr_t)text + (uint64_t)first * (uint64_t)recsize;
    const uintptr_t base = start & ~(uintptr_t)15;
    Staging s;
    s.shift = (int)(start - base);
    s.nvec = (s.shift + nrec * recsize + 15) >> 4;
    s.src = (const uint4 *)base;
    return s;
}

// The workgroup's records into LDS with aligned 16-byte loads.  Returns the position of the first
// record's first byte in s_text.
template <int kThreads>
__device__ __forceinline__ int stage_records(uint4 *s_text, const uint8_t *text, int64_t first,
                                             int nrec, int recsize)
{
    const Staging s = staging(text, first, nrec, recsize);
    for (int i = threadIdx.x; i < s.nvec; i += kThreads)
        s_text[i] = s.src[i];
    __syncthreads();
    return s.shift;
}

__device__ __forceinline__ void count_flagged(uint32_t flags, int32_t *nflagged)
{
    if (flags)
        atomicAdd(nflagged, 1);           // the compiler makes one add per wavefront of it
}

__device__ __forceinline__ bool is_space(uint32_t c)
{
    return c == ' ' || (c >= 9 && c <= 13);           // what bytes.split() splits at
}

// the LDS request of a workgroup of `records` records
inline int lds_bytes(int records, int recsize)
{
    return (15 + records * recsize + kSlack + 15) & ~15;
}

}  // namespace pb_text
