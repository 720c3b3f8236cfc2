// oligo_thermo_core.hpp -- the nearest-neighbour sums of one site of the oligo search, free of anything a GPU
// has: what k_ol_scan<true> does with a hit and what a thread of k_ol_thermo_best and of k_ol_thermo_sites does with a window.  Plain
// functions, host and device, so that a CPU program can run them against tests/tools/oligo_thermo_host.py.  Integers only: the tables
// are the caller's, nothing here multiplies by a temperature.
//
//   window   the site's L bases as the two planes the scan keeps: bit k of lo / hi is the low / high bit of the base k places before
//            the window's END (bit 0 = its last base)
//   pattern  the four mismatch planes of the oligo's row on the site's strand (oligo.hip: pattern_rows) -- bit k of plane b is set
//            iff base b is NOT in the set that faces the base k places before the end; on strand 1 that set is the complement of the
//            oligo's set at position k + 1
//   site     oligo position i = 1..L faces bit L - i on strand 0 and bit i - 1 on strand 1.  y_i, the base of the bound strand: the
//            complement of the text base on strand 0 (the oligo has the text's sense), the text base itself on strand 1.  x_i, the
//            oligo's base: 3 - y_i where the set holds it (the text base's mismatch bit is clear), else the least member of the set.
//            sum = init + end[0][x_1][y_1] + end[1][x_L][y_L] + the stacks [x_i][x_i+1][y_i][y_i+1], per plane dh, ds, dg, in int32.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OLT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define OLT_HD inline
#endif
// The walk over an oligo's positions stays a loop: unrolled it takes over 150 VGPRs and would cost the scan kernel its occupancy.
#if defined(__clang__)
#define OLT_NO_UNROLL _Pragma("nounroll")
#elif defined(__GNUC__)
#define OLT_NO_UNROLL _Pragma("GCC unroll 1")
#else
#define OLT_NO_UNROLL
#endif

namespace sw {
namespace olt {

constexpr uint32_t PLANES = 3, DH = 0, DS = 1, DG = 2;          // the planes of every table
constexpr uint32_t STACK_PLANE = 256, END_PLANE = 32;           // entries of a plane: [x1][x2][y1][y2], [side][x][y]
constexpr uint32_t STACK_WORDS = PLANES * STACK_PLANE, END_WORDS = PLANES * END_PLANE;
constexpr int32_t MAX_DG = 15000;                               // |dg| of an entry and of init: the sum over 31 stacks, 2 ends, init < 2^19
constexpr int32_t DG_BIAS = 1 << 19;
constexpr int32_t NO_SUM = INT32_MIN;                           // a signed field of a cell without a hit

struct Tables {
    const int16_t *stack;        // [3][4][4][4][4]
    const int16_t *end;          // [3][2][4][4]
    int32_t init[PLANES];
};

struct Sums {
    int32_t dh, ds, dg;
};

OLT_HD uint32_t base_at(const uint32_t *packed, uint64_t idx)
{
    return (packed[idx >> 4] >> (2 * (uint32_t)(idx & 15))) & 3u;
}

// the planes of the window of len bases whose first base has the batch-wide index idx (reads exactly the words that hold them)
OLT_HD void window(const uint32_t *packed, uint64_t idx, uint32_t len, uint32_t &lo, uint32_t &hi)
{
    lo = hi = 0;
    OLT_NO_UNROLL
    for (uint32_t j = 0; j < len; ++j) {
        const uint32_t b = base_at(packed, idx + j);
        lo = (lo << 1) | (b & 1u);
        hi = (hi << 1) | (b >> 1);
    }
}

// the mismatch bits of a window against a pattern: the plane of the text's base, place by place
OLT_HD uint32_t mismatches(uint32_t lo, uint32_t hi, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3)
{
    return (hi & ((lo & n3) | (~lo & n2))) | (~hi & ((lo & n1) | (~lo & n0)));
}

// x and y of the oligo position that faces bit k, as x << 2 | y
OLT_HD uint32_t pair_at(uint32_t lo, uint32_t hi, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t strand, uint32_t k)
{
    const uint32_t t = ((lo >> k) & 1u) | (((hi >> k) & 1u) << 1);
    const uint32_t out = ((n0 >> k) & 1u) | (((n1 >> k) & 1u) << 1) | (((n2 >> k) & 1u) << 2) | (((n3 >> k) & 1u) << 3);   // bases outside the facing set
    const uint32_t y = strand ? t : 3u - t;
    uint32_t x = 3u - y;
    if ((out >> t) & 1u) {
        // the set holds no partner: its least member.  Strand 0: the row's planes are the oligo's own, the lowest clear bit.  Strand 1:
        // plane b stands for the oligo's base 3 - b, the highest clear bit.  (A set is never empty: `out` is never 15.)
        const uint32_t in = ~out & 15u;
        const uint32_t low = (in & 1u) ? 0u : (in & 2u) ? 1u : (in & 4u) ? 2u : 3u;
        const uint32_t high = (in & 8u) ? 3u : (in & 4u) ? 2u : (in & 2u) ? 1u : 0u;
        x = strand ? 3u - high : low;
    }
    return (x << 2) | y;
}

// The sums of a site.  ALL = false: dg alone (dh and ds come back as 0).  len in 8..32.
template <bool ALL>
OLT_HD Sums site(uint32_t lo, uint32_t hi, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t len, uint32_t strand, const Tables &T)
{
    // the walk goes from the oligo's position 1 to L: bit L - 1 down to 0 on strand 0, bit 0 up to L - 1 on strand 1
    const uint32_t k1 = strand ? 0u : len - 1;
    uint32_t prev = pair_at(lo, hi, n0, n1, n2, n3, strand, k1);
    Sums s{ALL ? T.init[DH] : 0, ALL ? T.init[DS] : 0, T.init[DG]};
    {
        const uint32_t e = prev;                       // end[0][x_1][y_1]
        if (ALL) {
            s.dh += T.end[DH * END_PLANE + e];
            s.ds += T.end[DS * END_PLANE + e];
        }
        s.dg += T.end[DG * END_PLANE + e];
    }
    OLT_NO_UNROLL
    for (uint32_t i = 1; i < len; ++i) {
        const uint32_t k = strand ? i : len - 1 - i;
        const uint32_t cur = pair_at(lo, hi, n0, n1, n2, n3, strand, k);
        const uint32_t at = ((prev >> 2) << 6) | ((cur >> 2) << 4) | ((prev & 3u) << 2) | (cur & 3u);   // [x_i][x_i+1][y_i][y_i+1]
        if (ALL) {
            s.dh += T.stack[DH * STACK_PLANE + at];
            s.ds += T.stack[DS * STACK_PLANE + at];
        }
        s.dg += T.stack[DG * STACK_PLANE + at];
        prev = cur;
    }
    {
        const uint32_t e = 16u + prev;                 // end[1][x_L][y_L]
        if (ALL) {
            s.dh += T.end[DH * END_PLANE + e];
            s.ds += T.end[DS * END_PLANE + e];
        }
        s.dg += T.end[DG * END_PLANE + e];
    }
    return s;
}

}  // namespace olt
}  // namespace sw
