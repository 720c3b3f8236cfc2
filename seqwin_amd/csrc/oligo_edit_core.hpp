// oligo_edit_core.hpp -- the arithmetic of the oligo search with indels, free of anything a GPU has: what a
// lane of k_ole_scan does with its 16 ends and what a thread of k_ole_resolve does with a candidate.  Plain functions, host and device,
// so that a CPU program can run them against tests/tools/oligo_edit_host.py.
//
// Coordinates are DIRECTIONAL: on strand 0 a run T of n bases is read left to right, u = the base's offset in the run; on strand 1 it
// is the run's reverse complement that is read, u = n - 1 - offset and every base complemented.  An end e in 1..n is the number of
// bases read.  The pattern is the oligo on both strands.
//
//   row (8 words)  Eq planes 0..3 of the oligo -- bit i of plane b: base b lies in the set of position i --, L, three of padding
//   OleStream      up to 64 bases of the lane's neighbourhood as two 64-bit planes, bit t = the base at u = u0 + t
//   ole_scan       Myers' bit-vector column per base over Q = P[:L - c], started L + 2 d bases before the lane's first end minus d
//                  (every value <= d is then exact), the score of row |Q| per step; the clamp as a shift-and automaton over the last c
//                  bases; D(e) of the last 2 d + 1 ends as 3-bit fields of a word; the local-minimum rule on them
//   ole_align      the |Q| x (|Q| + d + 1) matrix of a candidate as the columns' vertical delta words, the canonical traceback on it
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OLE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define OLE_HD inline
#endif

namespace sw {
namespace ole {

constexpr uint32_t ROW = 8;                 // words of a pattern row
constexpr uint32_t MAX_EDITS = 4, MAX_LEN = 32, MAX_CLAMP = 8;
constexpr uint32_t FILL = 0x1249249u;       // nine 3-bit fields of value 1
constexpr uint32_t ALIGN_COLS = MAX_LEN + MAX_EDITS + 2;

OLE_HD uint32_t base_at(const uint32_t *packed, uint64_t idx)
{
    return (packed[idx >> 4] >> (2 * (uint32_t)(idx & 15))) & 3u;
}

// the base at directional offset u of a run (its first base at batch-wide index run_base, n bases)
OLE_HD uint32_t dir_base(const uint32_t *packed, uint64_t run_base, uint32_t n, uint32_t strand, uint32_t u)
{
    return strand ? 3u - base_at(packed, run_base + (n - 1 - u)) : base_at(packed, run_base + u);
}

OLE_HD uint32_t select4(uint32_t b0, uint32_t b1, uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3)
{
    const uint32_t lo = 0u - b0, hi = 0u - b1;
    return (hi & ((lo & e3) | (~lo & e2))) | (~hi & ((lo & e1) | (~lo & e0)));
}

OLE_HD uint32_t low_bits(uint32_t n)   // (n <= 32)
{
    return n >= 32 ? ~0u : (1u << n) - 1;
}

struct Myers {
    uint32_t pv, mv, score;
    OLE_HD void start(uint32_t rows)
    {
        pv = ~0u;
        mv = 0;
        score = rows;
    }
    // one text base whose match word is eq; top = the bit of the last row.  The first row's horizontal delta is 0: a match may start anywhere
    OLE_HD void step(uint32_t eq, uint32_t top)
    {
        const uint32_t xv = eq | mv;
        const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
        uint32_t ph = mv | ~(xh | pv);
        uint32_t mh = pv & xh;
        score += (ph & top) ? 1u : 0u;
        score -= (mh & top) ? 1u : 0u;
        ph <<= 1;
        mh <<= 1;
        pv = mh | ~(xv | ph);
        mv = ph & xv;
    }
};

// the lane's directional ends [a, a + cnt): strand 0 ends first + k .. ; strand 1 the starts first .. first + cnt - 1 as ends n - start
OLE_HD uint32_t first_end(uint32_t strand, uint32_t n, uint32_t k, uint32_t first, uint32_t cnt)
{
    return strand ? n - first - cnt + 1 : first + k;
}

struct OleStream {
    uint64_t lo, hi;
    uint32_t u0, u1;   // the bases [u0, u1) of the run, u1 - u0 <= 59
};

OLE_HD OleStream load_stream(const uint32_t *packed, uint64_t run_base, uint32_t n, uint32_t strand, uint32_t a, uint32_t cnt, uint32_t d)
{
    OleStream s;
    const uint32_t back = 2 * d + MAX_LEN;
    s.u0 = a > back ? a - back : 0;
    s.u1 = a + cnt - 1 + d < n ? a + cnt - 1 + d : n;
    s.lo = s.hi = 0;
    for (uint32_t t = 0; s.u0 + t < s.u1; ++t) {
        const uint64_t b = dir_base(packed, run_base, n, strand, s.u0 + t);
        s.lo |= (b & 1) << t;
        s.hi |= (b >> 1) << t;
    }
    return s;
}

// bit x of the result: the end a + x is a site of the oligo (row: its Eq planes; L its length) within d edits and a clamp of c
OLE_HD uint32_t ole_scan(const OleStream &s, uint32_t a, uint32_t cnt, uint32_t n, uint32_t d, uint32_t c, uint32_t L, uint32_t e0, uint32_t e1,
                         uint32_t e2, uint32_t e3)
{
    const uint32_t m = L - c, qmask = low_bits(m), top = 1u << (m - 1), cmask = (1u << c) - 1;
    const uint32_t q0 = e0 & qmask, q1 = e1 & qmask, q2 = e2 & qmask, q3 = e3 & qmask;
    const uint32_t back = 2 * d + L;
    uint32_t begin = a > back ? a - back : 0;    // the column the matrix starts at
    if (begin < s.u0) begin = s.u0;              // (never: u0 is the least begin of any length)
    const uint32_t last = a + cnt - 1 + d;       // the last end whose D is asked for; beyond n it is d + 1
    uint64_t wl = s.lo >> (begin - s.u0), wh = s.hi >> (begin - s.u0);
    Myers M;
    M.start(m);
    uint32_t hist = (d + 1) * FILL;              // field x: min(score, d + 1) of the column x steps back
    uint32_t win = (d + 1) * FILL;               // field x: D of the end x steps back
    uint32_t clamp = 0, cand = 0;
    for (uint32_t e = begin + 1; e <= last; ++e) {
        uint32_t dv = d + 1;
        if (e <= n) {
            const uint32_t b0 = (uint32_t)wl & 1u, b1 = (uint32_t)wh & 1u;
            wl >>= 1;
            wh >>= 1;
            M.step(select4(b0, b1, q0, q1, q2, q3), top);
            hist = (hist << 3) | (M.score < d + 1 ? M.score : d + 1);
            if (c) clamp = ((clamp << 1) | 1u) & (select4(b0, b1, e0, e1, e2, e3) >> m) & cmask;   // (c > 0: m < 32)
            const bool held = c == 0 || ((clamp >> (c - 1)) & 1u);
            if (held) dv = (hist >> (3 * c)) & 7u;
        }
        win = (win << 3) | dv;
        const uint32_t v = (win >> (3 * d)) & 7u;   // D of the end e - d
        if (v <= d && e >= a + d && e - d < a + cnt) {
            bool site = true;
            for (uint32_t x = 1; x <= d; ++x) {
                site = site && ((win >> (3 * (d + x))) & 7u) > v;    // the d ends before
                site = site && ((win >> (3 * (d - x))) & 7u) >= v;   // the d ends after
            }
            if (site) cand |= 1u << (e - d - a);
        }
    }
    return cand;
}

struct OleSite {
    uint32_t b, dist, mismatch, gaps;   // b: the directional start
};

// the alignment of the site that ends at e (directional).  The matrix starts |Q| + d + 1 columns before e - c, bounded by the run's start
OLE_HD OleSite ole_align(const uint32_t *packed, uint64_t run_base, uint32_t n, uint32_t strand, uint32_t e, uint32_t d, uint32_t c, uint32_t L,
                         const uint32_t eq[4])
{
    const uint32_t m = L - c, qmask = low_bits(m), top = 1u << (m - 1);
    const uint32_t je = e - c, span = m + d + 1;
    const uint32_t s = je > span ? je - span : 0, ncol = je - s;   // (ncol <= span <= 37)
    uint32_t pv[ALIGN_COLS], mv[ALIGN_COLS];
    Myers M;
    M.start(m);
    pv[0] = qmask;
    mv[0] = 0;
    for (uint32_t x = 1; x <= ncol; ++x) {
        M.step(eq[dir_base(packed, run_base, n, strand, s + x - 1)] & qmask, top);
        pv[x] = M.pv & qmask;
        mv[x] = M.mv & qmask;
    }
    auto D = [&](uint32_t i, uint32_t x) -> int {
        const uint32_t rows = low_bits(i);
        return (int)__builtin_popcount(pv[x] & rows) - (int)__builtin_popcount(mv[x] & rows);
    };
    OleSite out{0, (uint32_t)D(m, ncol), 0, 0};
    uint32_t i = m, x = ncol;
    for (uint32_t it = 0; i > 0 && it < 2 * ALIGN_COLS; ++it) {
        const int here = D(i, x);
        if (x > 0 && ((eq[dir_base(packed, run_base, n, strand, s + x - 1)] >> (i - 1)) & 1u)) {
            --i, --x;
        } else if (x > 0 && D(i - 1, x - 1) + 1 == here) {
            --i, --x, ++out.mismatch;
        } else if (D(i - 1, x) + 1 == here || x == 0) {
            --i, ++out.gaps;
        } else {
            --x, ++out.gaps;
        }
    }
    out.b = s + x;
    return out;
}

}  // namespace ole
}  // namespace sw
