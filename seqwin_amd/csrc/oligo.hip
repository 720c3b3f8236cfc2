// oligo.hip -- every place in every assembly of a resident batch where a short oligo (a primer, a probe) binds with at most d
// mismatches, on either strand: Hamming distance under IUPAC sets, exhaustive -- every window of the batch against every oligo.
//
// It has no counterpart in the reference, it is NOT BLAST (no e-values), and it fills none of MarkerMetrics.  DESIGN.md section 3.2j
// is the specification; tests/tools/oligo_host.py restates it twice.  A site is a Hamming site; what a caller's nearest-neighbour
// model says about it is an addition behind the hit (below, section 3.2o) -- integers on the caller's tables, no Tm on the device.
//
//   host           an oligo of L = 8..32 letters is L sets of bases.  Per oligo and strand one row of the pattern table (8 words):
//                  four MISMATCH planes -- bit t of plane b is set iff base b is NOT in the set that faces the text base t places
//                  before the window's END, for t < L; the length mask is folded into them --, the 3'-clamp mask and L.  Strand 1
//                  is the reverse complement: its set at t is the complement of the oligo's set at position t.
//   k_ol_scan      the hot path.  ONE walk for all lengths, windows indexed by their end: the runs of Lmin bases or more (Lmin = the
//                  shortest oligo of the call) cut into kmer_walk.hpp's tiles, a wave per tile, 16 consecutive window ends per lane.
//                  A lane keeps the last 32 bases as two 32-bit planes (the low and the high bit of every base; bit 0 = the end) and
//                  pre-rolls up to 31 bases before its first end, bounded by the run's start.  Per pattern (a wave-uniform loop; the
//                  table row arrives by scalar loads) and window: a bitwise select of the four planes by the text's two gives the
//                  mismatch bits in three operations, then popcount, the clamp, the comparison.  Candidates are rare; a wave that
//                  has one (a ballot) checks it against the run's start -- an oligo of L bases that ends at offset e of its run is
//                  a site iff e + 1 >= L --, counts it (atomicAdd), offers it as the best site (64-bit atomicMin) and appends it to
//                  the site buffer (wave_append).  All three are order-independent.
//   k_ol_resolve   the best site's key -> mm, record, pos, strand of a cell
//   k_ol_decode    a sorted site key -> assembly, record, pos (a template over where the key keeps the base index: both routes)
// With a thermodynamic model (tests/tools/oligo_thermo_host.py; oligo_thermo_core.hpp holds the site sum):
//   k_ol_scan<true>     the same walk; behind the candidate ballot, where mm is recomputed per hit anyway, it also sums the site's
//                       dg, counts it where dg <= max_dg (atomicAdd) and offers it as the most stable site (a second 64-bit
//                       atomicMin).  The tables (1.6 KB, divergent indices) are read from global memory through L1, not staged
//                       in LDS: hits are rare and k_ol_scan<false> must stay as it is.  No A/B of the two exists.
//   k_ol_thermo_best    the stable key -> the seven stable fields of a cell; it re-reads the window for dh, ds and mm
//   k_ol_thermo_sites   a sorted site key -> dh, ds, dg of the site; it re-reads L bases of the packed batch
// k_ol_scan<false> is the kernel without a model: a call without one launches what it launched before and allocates nothing more.
// Oligos are taken in groups (a pass over the batch each), assemblies in chunks bounded by the site buffer: a chunk that overflows
// is redone in two halves, one assembly that overflows has the buffer doubled -- as hits.hip treats its key buffer.
//
// With max_edits the same object is made by a second route (tests/tools/oligo_edit_host.py): unit-cost edit
// distance in place of the mismatch count, so that a site with a one-base bulge is found.  oligo_edit_core.hpp holds its arithmetic.
//   k_ole_scan     the tiles cover the runs of Lmin - d bases or more.  A lane owns the same 16 places of a tile twice: as ends on
//                  strand 0 and as starts -- the ends of the reverse complement -- on strand 1.  Per strand it keeps up to 59 bases
//                  around them as two 64-bit planes, in reading order; per oligo (a uniform loop, the Eq row by scalar loads) it steps
//                  Myers' column over them and applies the local-minimum rule in registers.  A candidate is appended as
//                  (oligo, strand, a base of the run that names the end).
//   k_ole_resolve  a thread per candidate: the small matrix and the canonical traceback give pos, end, mismatch and gaps; the site is
//                  counted, offered as the cell's best (64-bit atomicMin) and its buffer entry becomes the sortable site key
//   k_ole_best     the best site's key -> the seven best fields of a cell;  k_ol_decode with this route's shift: the list's columns
#include "screen_core.hpp"
#include "oligo_edit_core.hpp"
#include "oligo_thermo_core.hpp"
#include "oligo_result.hpp"

namespace sw {
namespace {

constexpr uint32_t OL_MIN_LEN = 8, OL_MAX_LEN = 32, OL_MAX_OLIGOS = 4096, OL_MAX_MM = 8, OL_MAX_CLAMP = 8;
constexpr uint32_t OL_ROW = 8;                         // words of a pattern row: planes 0..3, clamp, L, two of padding (32 B)
constexpr uint32_t OL_GROUP = OL_MAX_OLIGOS;           // oligos per pass: the table is read by scalar loads, nothing on the chip bounds it
constexpr uint64_t OL_BUFFER_BYTES = 64ull << 20;      // budget of the site buffer: speed only, chosen without a measurement
constexpr uint64_t OL_MAX_BASES = 1ull << 43;          // the batch-wide base index has 43 bits in a site key
constexpr uint64_t OL_MAX_SITES = 1ull << 32;
constexpr unsigned long long OL_NONE = ~0ull;
// best-site key: mm << 58 | base index << 1 | strand; site key: oligo << 48 | base index << 5 | strand << 4 | mm
constexpr uint32_t OL_BEST_MM_SHIFT = 58, OL_SITE_IDX_SHIFT = 5;   // (OL_SITE_Q_SHIFT: oligo_result.hpp)
// stable-site key: (dg + 2^19) << 44 | base index << 1 | strand -- 20 + 43 + 1 bits
constexpr uint32_t OL_STABLE_DG_SHIFT = 44;
static_assert(OL_MAX_BASES == 1ull << (OL_STABLE_DG_SHIFT - 1), "the stable key keeps the base index below the biased dg");
static_assert((OL_MAX_LEN + 2) * olt::MAX_DG < olt::DG_BIAS, "the biased dg of the longest oligo is positive and has 20 bits");

typedef const __attribute__((address_space(4))) uint32_t *ol_table_t;   // constant address space: uniform reads are scalar loads

struct ScanArgs {
    RunView v;                       // the tiles of this launch (runs of lmin bases or more; a "k-mer" is a window end)
    const uint32_t *tab;             // [n_pat][OL_ROW] the pass's patterns: 2 q' + strand
    uint32_t n_pat, q0;              // q0: the pass's first oligo
    uint32_t lmin, max_mm;
    uint64_t n_asm;
    uint32_t *n_sites;               // [n_oligos][n_asm]
    unsigned long long *best;        // [oligos of the pass][n_asm]
    unsigned long long *buf;         // site keys of the chunk (nullptr: no list is wanted; the cursor still counts)
    unsigned long long cap;
    unsigned long long *cursor;      // sites appended (above cap: the chunk overflowed, it is redone)
};

// what k_ol_scan<true> takes besides: the model and the cells it fills
struct ThermoScanArgs : ScanArgs {
    olt::Tables model;               // (device pointers)
    int32_t max_dg;                  // a hit with dg <= max_dg is stable (INT32_MAX: every hit)
    uint32_t *n_stable;              // [n_oligos][n_asm]
    unsigned long long *stable;      // [oligos of the pass][n_asm]
};

// the last 32 bases a lane has read, as the plane of their low bits and the plane of their high bits; bit 0 = the last base
struct PlaneRoller {
    const uint32_t *packed;
    uint64_t pos = 0;
    uint32_t w = 0, left = 0, lo = 0, hi = 0;
    __device__ __forceinline__ explicit PlaneRoller(const uint32_t *packed_bases) : packed(packed_bases) {}
    __device__ __forceinline__ void start(uint64_t pos0)   // (reads the word that holds base pos0)
    {
        pos = pos0;
        w = packed[pos >> 4] >> (2 * (uint32_t)(pos & 15));
        left = 16 - (uint32_t)(pos & 15);
    }
    __device__ __forceinline__ void roll()
    {
        if (left == 0) {
            w = packed[pos >> 4];
            left = 16;
        }
        lo = (lo << 1) | (w & 1u);
        hi = (hi << 1) | ((w >> 1) & 1u);
        w >>= 2;
        --left;
        ++pos;
    }
};

__device__ __forceinline__ uint32_t ol_select(uint32_t s, uint32_t one, uint32_t zero)
{
    return (s & one) | (~s & zero);
}

// the mismatch bits of a window (its two planes) against a pattern (its four mismatch planes)
__device__ __forceinline__ uint32_t ol_mismatches(uint32_t lo, uint32_t hi, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3)
{
    return ol_select(hi, ol_select(lo, n3, n2), ol_select(lo, n1, n0));
}

template <bool THERMO> __global__ __launch_bounds__(KW_TPB) void k_ol_scan(typename std::conditional<THERMO, ThermoScanArgs, ScanArgs>::type g)
{
    const uint32_t lane = threadIdx.x % KW_WAVE;
    uint32_t r, n_mine;
    uint64_t first;
    if (!wave_tile(g.v, lane, r, first, n_mine)) return;   // (the whole wave)
    if (g.buf && *(volatile unsigned long long *)g.cursor > g.cap) return;   // (the whole wave: the chunk has overflowed, it is redone anyway)
    const uint32_t a = g.v.run_asm[r];
    const uint64_t run_base = g.v.run_base[r];
    const uint64_t e0 = first + g.lmin - 1;   // the offset in the run of the lane's first window end
    uint32_t lo[KW_L], hi[KW_L];
    PlaneRoller R(g.v.packed);
    if (n_mine) {
        const uint32_t pre = e0 < OL_MAX_LEN - 1 ? (uint32_t)e0 : OL_MAX_LEN - 1;   // bases before the first end, bounded by the run's start
        R.start(run_base + e0 - pre);
        for (uint32_t i = 0; i < pre; ++i) R.roll();
    }
#pragma unroll
    for (uint32_t j = 0; j < KW_L; ++j) {
        if (j < n_mine) R.roll();
        lo[j] = R.lo;
        hi[j] = R.hi;
    }
    const uint32_t mine = (1u << n_mine) - 1;   // (n_mine <= 16)
    const ol_table_t tab = (ol_table_t)g.tab;
    for (uint32_t p = 0; p < g.n_pat; ++p) {    // (uniform)
        const ol_table_t row = tab + (uint64_t)p * OL_ROW;
        const uint32_t n0 = row[0], n1 = row[1], n2 = row[2], n3 = row[3], clamp = row[4], len = row[5];
        uint32_t cand = 0;
#pragma unroll
        for (uint32_t j = 0; j < KW_L; ++j) {
            const uint32_t x = ol_mismatches(lo[j], hi[j], n0, n1, n2, n3);
            cand |= ((uint32_t)__popc(x) <= g.max_mm && !(x & clamp)) ? 1u << j : 0u;
        }
        if (!__ballot(cand != 0)) continue;     // (uniform) candidates are rare
        // a window that ends at offset e of its run holds the oligo iff e + 1 >= len
        cand &= mine;
        if (e0 + 1 < len) {
            const uint32_t short_by = len - 1 - (uint32_t)e0;   // (1..31) the lane's first short_by ends lie too near the run's start
            cand &= short_by >= KW_L ? 0u : ~((1u << short_by) - 1);
        }
        const WaveRange w = wave_append(g.cursor, lane, (uint32_t)__popc(cand));
        if (!w.total) continue;                 // (uniform)
        const bool store = g.buf && w.base + w.total <= g.cap;   // (uniform) overflow: the host reads it from the cursor
        const uint32_t q_local = p >> 1, strand = p & 1;
        uint32_t at = 0;
#pragma unroll
        for (uint32_t j = 0; j < KW_L; ++j) {
            if (!((cand >> j) & 1)) continue;
            const unsigned long long mm = (unsigned long long)__popc(ol_mismatches(lo[j], hi[j], n0, n1, n2, n3));
            const unsigned long long idx = run_base + e0 + j + 1 - len;   // the batch-wide index of the site's first base
            atomicAdd(g.n_sites + (uint64_t)(g.q0 + q_local) * g.n_asm + a, 1u);
            atomicMin(g.best + (uint64_t)q_local * g.n_asm + a, (mm << OL_BEST_MM_SHIFT) | (idx << 1) | strand);
            if (store)
                g.buf[w.base + w.offset + at] = ((unsigned long long)(g.q0 + q_local) << OL_SITE_Q_SHIFT) | (idx << OL_SITE_IDX_SHIFT) | (strand << 4) | mm;
            ++at;
        }
        if constexpr (THERMO) {
            // the model's part, hit by hit in a loop of its own: one copy of the walk over the oligo's positions, not one per place
            // of the lane (16 copies cost 254 VGPRs).  No wave operation inside, so the lanes may leave it apart.
            for (uint32_t rest = cand; rest; rest &= rest - 1) {
                const uint32_t j = (uint32_t)__ffs(rest) - 1;
                uint32_t l = lo[0], h = hi[0];
#pragma unroll
                for (uint32_t x = 1; x < KW_L; ++x) {
                    l = j == x ? lo[x] : l;
                    h = j == x ? hi[x] : h;
                }
                const int32_t dg = olt::site<false>(l, h, n0, n1, n2, n3, len, strand, g.model).dg;
                const unsigned long long idx = run_base + e0 + j + 1 - len;
                if (dg <= g.max_dg) atomicAdd(g.n_stable + (uint64_t)(g.q0 + q_local) * g.n_asm + a, 1u);
                atomicMin(g.stable + (uint64_t)q_local * g.n_asm + a,
                          ((unsigned long long)(uint32_t)(dg + olt::DG_BIAS) << OL_STABLE_DG_SHIFT) | (idx << 1) | strand);
            }
        }
    }
}

// the last run whose first base is <= idx
__device__ __forceinline__ uint32_t ol_run_of(const uint64_t *__restrict__ run_base, uint32_t n_runs, uint64_t idx)
{
    uint32_t lo = 0, hi = n_runs;
    while (lo + 1 < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (run_base[mid] <= idx) lo = mid; else hi = mid;
    }
    return lo;
}

// cell i of the pass (oligo q0 + i / n_asm, assembly i % n_asm) with a site: the four fields of its best one
__global__ __launch_bounds__(SCR_TPB) void k_ol_resolve(uint64_t base, uint64_t end, const unsigned long long *__restrict__ best, uint64_t cell0, RunView v,
                                                        uint32_t *__restrict__ mm, uint32_t *__restrict__ rec, uint32_t *__restrict__ pos,
                                                        uint32_t *__restrict__ strand)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end) return;
    const unsigned long long key = best[i];
    if (key == OL_NONE) return;   // (the fields hold 0xFFFFFFFF)
    const uint64_t idx = (key & ((1ull << OL_BEST_MM_SHIFT) - 1)) >> 1;
    const uint32_t r = ol_run_of(v.run_base, v.n_runs, idx);
    mm[cell0 + i] = (uint32_t)(key >> OL_BEST_MM_SHIFT);
    rec[cell0 + i] = v.run_rec[r];
    pos[cell0 + i] = v.run_pos[r] + (uint32_t)(idx - v.run_base[r]);
    strand[cell0 + i] = (uint32_t)(key & 1);
}

// sorted site key i of either route -> assembly, record, pos; the key holds the base index in its bits [IDX_SHIFT, IDX_SHIFT + IDX_BITS)
template <uint32_t IDX_SHIFT, uint32_t IDX_BITS>
__global__ __launch_bounds__(SCR_TPB) void k_ol_decode(uint64_t base, uint64_t end, const uint64_t *__restrict__ keys, RunView v, uint32_t *__restrict__ asm_out,
                                                       uint32_t *__restrict__ rec, uint32_t *__restrict__ pos)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end) return;
    const uint64_t idx = (keys[i] >> IDX_SHIFT) & ((1ull << IDX_BITS) - 1);
    const uint32_t r = ol_run_of(v.run_base, v.n_runs, idx);
    asm_out[i] = v.run_asm[r];
    rec[i] = v.run_rec[r];
    pos[i] = v.run_pos[r] + (uint32_t)(idx - v.run_base[r]);
}

struct StableFields {
    int32_t *dg, *dh, *ds;
    uint32_t *rec, *pos, *strand, *mm;
};

// cell i of the pass: the seven fields of its most stable site, or NO_HIT (the signed fields: INT32_MIN) without one
__global__ __launch_bounds__(SCR_TPB) void k_ol_thermo_best(uint64_t base, uint64_t end, const unsigned long long *__restrict__ stable, uint64_t cell0, RunView v,
                                                            const uint32_t *__restrict__ tab, uint64_t n_asm, olt::Tables model, StableFields f)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end) return;
    const unsigned long long key = stable[i];
    if (key == OL_NONE) {
        f.dg[cell0 + i] = f.dh[cell0 + i] = f.ds[cell0 + i] = olt::NO_SUM;
        f.rec[cell0 + i] = f.pos[cell0 + i] = f.strand[cell0 + i] = f.mm[cell0 + i] = 0xFFFFFFFFu;
        return;
    }
    const uint64_t idx = (key & ((1ull << OL_STABLE_DG_SHIFT) - 1)) >> 1;
    const uint32_t strand = (uint32_t)(key & 1);
    const uint32_t r = ol_run_of(v.run_base, v.n_runs, idx);
    const uint32_t *row = tab + ((i / n_asm) * 2 + strand) * OL_ROW;
    const uint32_t n0 = row[0], n1 = row[1], n2 = row[2], n3 = row[3], len = row[5];
    uint32_t lo, hi;
    olt::window(v.packed, idx, len, lo, hi);   // (a site lies inside its run: [idx, idx + len) are bases of the batch)
    const olt::Sums s = olt::site<true>(lo, hi, n0, n1, n2, n3, len, strand, model);
    f.dg[cell0 + i] = s.dg;                    // (= the key's dg)
    f.dh[cell0 + i] = s.dh;
    f.ds[cell0 + i] = s.ds;
    f.rec[cell0 + i] = v.run_rec[r];
    f.pos[cell0 + i] = v.run_pos[r] + (uint32_t)(idx - v.run_base[r]);
    f.strand[cell0 + i] = strand;
    f.mm[cell0 + i] = (uint32_t)__popc(olt::mismatches(lo, hi, n0, n1, n2, n3));
}

// sorted site key i: the sums of its site.  tab holds the rows of ALL oligos of the call
__global__ __launch_bounds__(SCR_TPB) void k_ol_thermo_sites(uint64_t base, uint64_t end, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ packed,
                                                             const uint32_t *__restrict__ tab, olt::Tables model, int32_t *__restrict__ dh,
                                                             int32_t *__restrict__ ds, int32_t *__restrict__ dg)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end) return;
    const uint64_t key = keys[i];
    const uint64_t idx = (key & ((1ull << OL_SITE_Q_SHIFT) - 1)) >> OL_SITE_IDX_SHIFT;   // (64 bits: the batch-wide index passes 2^32)
    const uint32_t q = (uint32_t)(key >> OL_SITE_Q_SHIFT), strand = (uint32_t)(key >> 4) & 1u;
    const uint32_t *row = tab + ((uint64_t)q * 2 + strand) * OL_ROW;
    const uint32_t len = row[5];
    uint32_t lo, hi;
    olt::window(packed, idx, len, lo, hi);
    const olt::Sums s = olt::site<true>(lo, hi, row[0], row[1], row[2], row[3], len, strand, model);
    dh[i] = s.dh;
    ds[i] = s.ds;
    dg[i] = s.dg;
}

// ---- the route with indels (section 3.2n) ---------------------------------------------------------------------------------------------
constexpr uint32_t OLE_MAX_EDITS = ole::MAX_EDITS;
constexpr uint64_t OLE_IDX_MASK = (1ull << 43) - 1;
// candidate: oligo of the pass << 44 | strand << 43 | a base of the run (strand 0: the end's last base, strand 1: the site's first)
constexpr uint32_t OLE_CAND_Q_SHIFT = 44, OLE_CAND_STRAND_SHIFT = 43;
// site key: oligo << 52 | index of pos << 9 | (end - pos - (L - d)) << 5 | strand << 4 | code;  code = 5 t + mismatch, gaps = |end - pos - L| + 2 t
// best key: dist << 61 | index of pos << 9 | strand << 8 | (end - pos - (L - d)) << 4 | code
constexpr uint32_t OLE_IDX_SHIFT = 9, OLE_BEST_DIST_SHIFT = 61;   // (OLE_SITE_Q_SHIFT: oligo_result.hpp)

struct EditScanArgs {
    RunView v;                       // the tiles of this launch (runs of k = lmin - d bases or more)
    const uint32_t *tab;             // [n_q][ole::ROW] the pass's oligos
    uint32_t n_q, k, d, c;
    unsigned long long *buf;         // candidates of the chunk
    unsigned long long cap;
    unsigned long long *cursor;      // candidates appended (above cap: the chunk overflowed, it is redone)
};

__global__ __launch_bounds__(KW_TPB) void k_ole_scan(EditScanArgs g)
{
    const uint32_t lane = threadIdx.x % KW_WAVE;
    uint32_t r, n_mine;
    uint64_t first;
    if (!wave_tile(g.v, lane, r, first, n_mine)) return;   // (the whole wave)
    if (*(volatile unsigned long long *)g.cursor > g.cap) return;   // (the whole wave: the chunk has overflowed, it is redone anyway)
    const uint64_t run_base = g.v.run_base[r];
    const uint32_t n = g.v.run_nk[r] + g.k - 1;           // bases of the run
    ole::OleStream S[2] = {};
    uint32_t a[2] = {0, 0};
    if (n_mine) {
#pragma unroll
        for (uint32_t s = 0; s < 2; ++s) {
            a[s] = ole::first_end(s, n, g.k, (uint32_t)first, n_mine);
            S[s] = ole::load_stream(g.v.packed, run_base, n, s, a[s], n_mine, g.d);
        }
    }
    const ol_table_t tab = (ol_table_t)g.tab;
    for (uint32_t q = 0; q < g.n_q; ++q) {      // (uniform)
        const ol_table_t row = tab + (uint64_t)q * ole::ROW;
        const uint32_t e0 = row[0], e1 = row[1], e2 = row[2], e3 = row[3], len = row[4];
#pragma unroll
        for (uint32_t s = 0; s < 2; ++s) {
            const uint32_t cand = n_mine ? ole::ole_scan(S[s], a[s], n_mine, n, g.d, g.c, len, e0, e1, e2, e3) : 0u;
            if (!__ballot(cand != 0)) continue;     // (uniform) candidates are rare
            const WaveRange w = wave_append(g.cursor, lane, (uint32_t)__popc(cand));
            if (!w.total || w.base + w.total > g.cap) continue;   // (uniform) overflow: the host reads it from the cursor
            uint32_t at = 0;
            for (uint32_t x = 0; x < KW_L; ++x) {
                if (!((cand >> x) & 1)) continue;
                const uint32_t e = a[s] + x;        // (1..n)
                const unsigned long long anchor = run_base + (s ? n - e : e - 1);
                g.buf[w.base + w.offset + at] = ((unsigned long long)q << OLE_CAND_Q_SHIFT) | ((unsigned long long)s << OLE_CAND_STRAND_SHIFT) | anchor;
                ++at;
            }
        }
    }
}

// candidate i of the chunk: its alignment; the site is counted, offered as its cell's best, and buf[i] becomes its site key
__global__ __launch_bounds__(SCR_TPB) void k_ole_resolve(uint64_t base, uint64_t end, unsigned long long *__restrict__ buf, const uint32_t *__restrict__ tab,
                                                         uint32_t q0, RunView v, uint32_t k, uint32_t d, uint32_t c, uint64_t n_asm,
                                                         uint32_t *__restrict__ n_sites, unsigned long long *__restrict__ best)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end) return;
    const unsigned long long raw = buf[i];
    const uint32_t ql = (uint32_t)(raw >> OLE_CAND_Q_SHIFT), s = (uint32_t)(raw >> OLE_CAND_STRAND_SHIFT) & 1u;
    const uint64_t anchor = raw & OLE_IDX_MASK;
    const uint32_t r = ol_run_of(v.run_base, v.n_runs, anchor);
    const uint64_t run_base = v.run_base[r];
    const uint32_t n = v.run_nk[r] + k - 1, off = (uint32_t)(anchor - run_base);
    const uint32_t e = s ? n - off : off + 1;
    const uint32_t *row = tab + (uint64_t)ql * ole::ROW;
    const uint32_t eq[4] = {row[0], row[1], row[2], row[3]}, len = row[4];
    const ole::OleSite site = ole::ole_align(v.packed, run_base, n, s, e, d, c, len, eq);
    const uint32_t pos = s ? n - e : site.b, stop = s ? n - site.b : e;
    const uint32_t over = (stop - pos - (len - d)) & 15u;                    // (0..2 d)
    const uint32_t skew = over > d ? over - d : d - over;                    // |#D - #I|
    const uint32_t code = 5 * ((site.gaps - skew) >> 1) + site.mismatch;     // (gaps = skew + 2 t, t <= 2, mismatch <= 4)
    const unsigned long long idx = run_base + pos, low = ((unsigned long long)over << 4) | code;
    const uint64_t a = v.run_asm[r];
    atomicAdd(n_sites + (uint64_t)(q0 + ql) * n_asm + a, 1u);
    atomicMin(best + (uint64_t)ql * n_asm + a, ((unsigned long long)site.dist << OLE_BEST_DIST_SHIFT) | (idx << OLE_IDX_SHIFT) | ((unsigned long long)s << 8) | low);
    buf[i] = ((unsigned long long)(q0 + ql) << OLE_SITE_Q_SHIFT) | (idx << OLE_IDX_SHIFT) | ((unsigned long long)over << 5) | ((unsigned long long)s << 4) | code;
}

struct BestFields {
    uint32_t *dist, *rec, *pos, *strand, *end, *mismatch, *gaps;
};

// cell i of the pass with a site: the seven fields of its best one
__global__ __launch_bounds__(SCR_TPB) void k_ole_best(uint64_t base, uint64_t end, const unsigned long long *__restrict__ best, uint64_t cell0, RunView v,
                                                      const uint32_t *__restrict__ tab, uint64_t n_asm, uint32_t d, BestFields f)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end) return;
    const unsigned long long key = best[i];
    if (key == OL_NONE) return;   // (the fields hold 0xFFFFFFFF)
    const uint64_t idx = (key >> OLE_IDX_SHIFT) & OLE_IDX_MASK;
    const uint32_t r = ol_run_of(v.run_base, v.n_runs, idx);
    const uint32_t len = tab[(i / n_asm) * ole::ROW + 4], over = (uint32_t)(key >> 4) & 15u, code = (uint32_t)key & 15u;
    const uint32_t pos = v.run_pos[r] + (uint32_t)(idx - v.run_base[r]);
    f.dist[cell0 + i] = (uint32_t)(key >> OLE_BEST_DIST_SHIFT);
    f.rec[cell0 + i] = v.run_rec[r];
    f.pos[cell0 + i] = pos;
    f.strand[cell0 + i] = (uint32_t)(key >> 8) & 1u;
    f.end[cell0 + i] = pos + len - d + over;
    f.mismatch[cell0 + i] = code % 5;
    f.gaps[cell0 + i] = (over > d ? over - d : d - over) + 2 * (code / 5);
}

// ---- host: the oligos -------------------------------------------------------------------------------------------------------------
// the set of bases a letter stands for (bit b: base b of A C G T), 0: no letter of an oligo
uint32_t iupac_set(unsigned char c)
{
    switch (c | 0x20) {
    case 'a': return 1;
    case 'c': return 2;
    case 'g': return 4;
    case 't': case 'u': return 8;
    case 'r': return 1 | 4;
    case 'y': return 2 | 8;
    case 's': return 2 | 4;
    case 'w': return 1 | 8;
    case 'k': return 4 | 8;
    case 'm': return 1 | 2;
    case 'b': return 2 | 4 | 8;
    case 'd': return 1 | 4 | 8;
    case 'h': return 1 | 2 | 8;
    case 'v': return 1 | 2 | 4;
    case 'n': return 15;
    default: return 0;
    }
}

inline uint32_t complement_set(uint32_t s)   // A <-> T, C <-> G
{
    return ((s & 1) << 3) | ((s & 2) << 1) | ((s & 4) >> 1) | ((s & 8) >> 3);
}

// what a call says about its oligos by itself, before a device is touched; returns the shortest length
uint32_t check_oligos(const uint64_t *offsets, const char *blob, uint64_t n, uint64_t max_mm, uint64_t three_prime)
{
    if (n < 1 || n > OL_MAX_OLIGOS) raise(SW_ERR_VALUE, "oligo hits: %llu oligos; 1..%u are taken", (unsigned long long)n, OL_MAX_OLIGOS);
    if (!offsets || !blob) raise(SW_ERR_VALUE, "oligo hits: a NULL handle or array");
    if (offsets[0] != 0) raise(SW_ERR_VALUE, "oligo hits: offsets must start at 0");
    uint32_t lmin = OL_MAX_LEN;
    for (uint64_t q = 0; q < n; ++q) {
        if (offsets[q] > offsets[q + 1]) raise(SW_ERR_VALUE, "oligo hits: offsets must be non-decreasing (oligo %llu)", (unsigned long long)q);
        const uint64_t len = offsets[q + 1] - offsets[q];
        if (len < OL_MIN_LEN || len > OL_MAX_LEN)
            raise(SW_ERR_VALUE, "oligo hits: oligo %llu has %llu letters; %u..%u are taken", (unsigned long long)q, (unsigned long long)len, OL_MIN_LEN, OL_MAX_LEN);
        for (uint64_t i = offsets[q]; i < offsets[q + 1]; ++i)
            if (!iupac_set((unsigned char)blob[i]))
                raise(SW_ERR_VALUE, "oligo hits: oligo %llu holds byte 0x%02x at %llu, which is no IUPAC letter", (unsigned long long)q,
                      (unsigned)(unsigned char)blob[i], (unsigned long long)(i - offsets[q]));
        lmin = std::min<uint32_t>(lmin, (uint32_t)len);
    }
    if (max_mm > OL_MAX_MM || max_mm >= lmin)
        raise(SW_ERR_VALUE, "oligo hits: max_mismatch must lie in 0..%u and below the shortest oligo's %u letters (got %llu)", OL_MAX_MM, lmin,
              (unsigned long long)max_mm);
    if (three_prime > OL_MAX_CLAMP) raise(SW_ERR_VALUE, "oligo hits: three_prime must lie in 0..%u (got %llu)", OL_MAX_CLAMP, (unsigned long long)three_prime);
    return lmin;
}

// the two rows of oligo `text`: strand 0, strand 1
void pattern_rows(const char *text, uint32_t len, uint32_t clamp, uint32_t *rows)
{
    memset(rows, 0, 2 * OL_ROW * sizeof(uint32_t));
    for (uint32_t t = 0; t < len; ++t) {
        const uint32_t s0 = iupac_set((unsigned char)text[len - 1 - t]);       // strand 0: position len - 1 - t faces the base t before the end
        const uint32_t s1 = complement_set(iupac_set((unsigned char)text[t])); // strand 1: P1[len - 1 - t] = complement of P0[t]
        for (uint32_t b = 0; b < 4; ++b) {
            if (!((s0 >> b) & 1)) rows[b] |= 1u << t;
            if (!((s1 >> b) & 1)) rows[OL_ROW + b] |= 1u << t;
        }
    }
    const uint32_t c = clamp ? (uint32_t)((1ull << clamp) - 1) : 0u;   // (clamp <= 8 <= len)
    rows[4] = c;                       // strand 0: the oligo's last `clamp` positions = the window's last bases
    rows[OL_ROW + 4] = c << (len - clamp);   // strand 1: its first positions = the window's first bases
    rows[5] = rows[OL_ROW + 5] = len;
}

}  // namespace
}  // namespace sw

namespace sw {
namespace {

// a caller's model as sw_batch_oligo_hits_thermo takes it (host pointers)
struct ThermoModel {
    const int16_t *stack, *end;
    const int32_t *init;
    int32_t max_dg;                  // INT32_MAX: no threshold
};

// what a model says about itself, before a device is touched: the stable key relies on the bound of the dg plane
void check_model(const ThermoModel &m)
{
    if (!m.stack || !m.end || !m.init) raise(SW_ERR_VALUE, "oligo hits: a NULL handle or array");
    for (uint32_t i = 0; i < olt::STACK_PLANE; ++i)
        if (std::abs((int)m.stack[olt::DG * olt::STACK_PLANE + i]) > olt::MAX_DG)
            raise(SW_ERR_VALUE, "oligo hits: the model's dg of stack %u is %d; |dg| <= %d is taken", i, (int)m.stack[olt::DG * olt::STACK_PLANE + i], olt::MAX_DG);
    for (uint32_t i = 0; i < olt::END_PLANE; ++i)
        if (std::abs((int)m.end[olt::DG * olt::END_PLANE + i]) > olt::MAX_DG)
            raise(SW_ERR_VALUE, "oligo hits: the model's dg of end %u is %d; |dg| <= %d is taken", i, (int)m.end[olt::DG * olt::END_PLANE + i], olt::MAX_DG);
    if (m.init[olt::DG] > olt::MAX_DG || m.init[olt::DG] < -olt::MAX_DG)
        raise(SW_ERR_VALUE, "oligo hits: the model's dg of init is %d; |dg| <= %d is taken", (int)m.init[olt::DG], olt::MAX_DG);
}

// ---- the steps batch_oligo_hits and batch_oligo_edit share, each written once ------------------------------------------------------
struct OligoCounts {   // sw_oligos_stats, in its order
    uint64_t windows = 0, passes = 0, chunks = 0, launches = 0, hits = 0, grows = 0, splits = 0, comparisons = 0;
};
static_assert(sizeof(OligoCounts) == sizeof(sw_oligos::counters), "OligoCounts is copied into sw_oligos::counters");

// the start of a result: what the batch must be, the sizes, the oligos' lengths and the first n_fields cell fields (n_sites 0, the rest 0xFF)
void start_result(const sw_batch &b, const uint64_t *offsets, uint64_t nq, uint64_t max_mm, int64_t max_edits, uint32_t three_prime, bool want_sites, int n_fields,
                  hipStream_t stream, sw_oligos &o)
{
    const HostBatch &h = b.host;
    const uint64_t cells = nq * h.n_assemblies;
    if (h.rec_len.size() && !b.d_packed.p) raise(SW_ERR_VALUE, "oligo hits: the batch holds no packed bases (it must be resident)");
    if ((uint64_t)h.packed_words32() * 16 >= OL_MAX_BASES) raise(SW_ERR_RUNTIME, "oligo hits: the batch has 2^43 bases or more");
    o.nq = nq;
    o.n_asm = h.n_assemblies;
    o.max_mm = max_mm;
    o.max_edits = max_edits;               // (-1: a Hamming result)
    o.three_prime = three_prime;
    o.has_sites = want_sites;
    for (uint64_t q = 0; q < nq; ++q) o.lens.push_back((uint32_t)(offsets[q + 1] - offsets[q]));
    for (int f = 0; f < n_fields; ++f) {
        o.field[f].alloc(cells);
        if (cells) SW_HIP(hipMemsetAsync(o.field[f].p, f ? 0xFF : 0, cells * 4, stream));
    }
}

// how a call is cut: oligos per pass, entries of the buffer a chunk of assemblies may fill, workgroups per launch of the scan kernel;
// the three switches (test library) lower them
struct ChunkSizes {
    uint64_t group, cap;
    uint32_t blocks_max;
};

ChunkSizes chunk_sizes(uint64_t nq)
{
    uint64_t group = OL_GROUP, budget = OL_BUFFER_BYTES;
    if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_OLIGO_GROUP")) group = std::min<uint64_t>(std::max<uint64_t>(env_u64(e, group), 1), OL_GROUP);
    if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_OLIGO_BUFFER_KB")) budget = env_u64(e, budget >> 10) << 10;
    return {std::min<uint64_t>(group, nq), std::min<uint64_t>(std::max<uint64_t>(budget / 8, 1), OL_MAX_SITES), launch_blocks("SEQWIN_AMD_OLIGO_MAX_BLOCKS")};
}

// the chunk of assemblies [a0, a1) overflowed the buffer and is redone: in two halves (the first now, the second is the next chunk), or,
// one assembly above the budget, with the buffer doubled
void overflow_step(uint64_t a0, uint64_t a1, uint64_t &rows, uint64_t &cap, DevArray<unsigned long long> &buf, OligoCounts &c)
{
    if (a1 - a0 > 1) {
        rows = (a1 - a0 + 1) / 2;
        ++c.splits;
    } else {
        if (cap >= OL_MAX_SITES) raise(SW_ERR_RUNTIME, "oligo hits: assembly %llu alone has 2^32 sites or more", (unsigned long long)a0);
        cap = std::min<uint64_t>(cap * 2, OL_MAX_SITES);
        buf.alloc(cap);
        ++c.grows;
    }
}

typedef void (*DecodeKernel)(uint64_t, uint64_t, const uint64_t *, RunView, uint32_t *, uint32_t *, uint32_t *);   // an instantiation of k_ol_decode

// the site list: all chunks' keys in one ascending order -- (oligo, assembly, record, pos, strand), an edit result: (.., pos, end, strand)
// -- and the three columns the keys do not hold, by the route's instantiation of the decode kernel
void finish_site_list(std::vector<DevArray<uint64_t>> &lists, uint64_t hits, DecodeKernel decode, const RunView &v, hipStream_t stream, sw_oligos &o)
{
    DevArray<uint64_t> ka(hits), kb(hits);
    uint64_t at = 0;
    for (DevArray<uint64_t> &l : lists) {
        SW_HIP(hipMemcpyAsync(ka.p + at, l.p, l.n * 8, hipMemcpyDeviceToDevice, stream));
        at += l.n;
    }
    if (at != hits) raise(SW_ERR_RUNTIME, "internal error: the chunks' site lists do not add up");
    uint64_t *kp = ka.p, *ap = kb.p;
    sort_all_bits(kp, ap, hits, stream);
    lists.clear();
    if (kp != ka.p) std::swap(ka, kb);
    o.keys = std::move(ka);
    o.n_list = hits;
    o.s_asm.alloc(hits);
    o.s_rec.alloc(hits);
    o.s_pos.alloc(hits);
    launch_1d(decode, hits, stream, (const uint64_t *)o.keys.p, v, o.s_asm.p, o.s_rec.p, o.s_pos.p);
}

// the end of either route: the stream's last synchronisation, scan_ms -- e0 to e1 without what the route timed by events of its own
// (apart_ms) --, order_ms and the counters
void close_result(hipStream_t stream, const Event &e0, const Event &e1, const Event &e2, double apart_ms, const OligoCounts &c, sw_oligos &o)
{
    SW_HIP(hipStreamSynchronize(stream));   // (the temporaries go back to the pool behind the kernels)
    float ms = 0;
    SW_HIP(hipEventElapsedTime(&ms, e0, e1));
    o.ms[0] = std::max(0.0, (double)ms - apart_ms);
    SW_HIP(hipEventElapsedTime(&ms, e1, e2));
    o.ms[1] = ms;
    memcpy(o.counters, &c, sizeof c);
}

// what the creating entry points do behind their argument checks: search(o) fills a fresh result on the batch's device, inside the stream's scope
template <class F> void make_oligos(const sw_batch *batch, void *stream, sw_oligos **out, F &&search)
{
    if (!batch || !out) raise(SW_ERR_VALUE, "oligo hits: a NULL handle or array");
    require_device(batch->device, "the batch");
    StreamScope scope((hipStream_t)stream);
    std::unique_ptr<sw_oligos> o(new sw_oligos);
    o->device = batch->device;
    search(*o);
    *out = o.release();
}

// th: the model of a call with one (section 3.2o), else nullptr -- then nothing below differs from the search without it
void batch_oligo_hits(const sw_batch &b, const uint64_t *offsets, const char *blob, uint64_t nq, uint32_t lmin, uint32_t max_mm, uint32_t three_prime,
                      bool want_sites, hipStream_t stream, sw_oligos &o, const ThermoModel *th = nullptr)
{
    const HostBatch &h = b.host;
    const uint64_t n_asm = h.n_assemblies, cells = nq * n_asm;
    start_result(b, offsets, nq, max_mm, -1, three_prime, want_sites, 5, stream, o);
    DevArray<int16_t> d_model;               // the model's stack and end tables
    DevArray<uint32_t> all_rows;             // with the list: the pattern rows of every oligo (k_ol_thermo_sites)
    olt::Tables model{};
    if (th) {
        o.thermo = true;
        o.n_stable.alloc(cells);
        if (cells) SW_HIP(hipMemsetAsync(o.n_stable.p, 0, cells * 4, stream));
        for (int f = 0; f < 3; ++f) {        // (k_ol_thermo_best fills them; a batch without a run of lmin bases launches nothing)
            o.stable_sum[f].alloc(cells);
            if (cells) SW_HIP(hipMemsetD32Async((hipDeviceptr_t)o.stable_sum[f].p, (int)olt::NO_SUM, cells, stream));
        }
        for (int f = 0; f < 4; ++f) {
            o.stable_at[f].alloc(cells);
            if (cells) SW_HIP(hipMemsetAsync(o.stable_at[f].p, 0xFF, cells * 4, stream));
        }
        d_model.alloc(olt::STACK_WORDS + olt::END_WORDS);
        SW_HIP(hipMemcpyAsync(d_model.p, th->stack, olt::STACK_WORDS * 2, hipMemcpyHostToDevice, stream));
        SW_HIP(hipMemcpyAsync(d_model.p + olt::STACK_WORDS, th->end, olt::END_WORDS * 2, hipMemcpyHostToDevice, stream));
        model.stack = d_model.p;
        model.end = d_model.p + olt::STACK_WORDS;
        for (uint32_t i = 0; i < olt::PLANES; ++i) model.init[i] = th->init[i];
    }
    // ---- the runs of lmin bases or more: a tile's "k-mers" are window ends (kmer_walk.hpp) ----
    RunTiles T;
    build_run_tiles(h, lmin, "oligo hits", T);
    auto [group, cap, blocks_max] = chunk_sizes(nq);   // (cap doubles with the buffer)
    OligoCounts cnt;
    std::vector<DevArray<uint64_t>> lists;   // the chunks' site keys, in the order the chunks ended
    Event e0, e1, e2;
    std::unique_ptr<Event> ta, tb;           // the model's kernels are timed by events of their own: none without a model
    if (th) {
        ta.reset(new Event);
        tb.reset(new Event);
    }
    double best_ms = 0;
    SW_HIP(hipEventRecord(e0, stream));
    DevRunTiles runs(T, b.d_packed.p, stream, true);
    if (T.tiles && cells) {
        std::vector<uint32_t> rows_host(group * 2 * OL_ROW);
        DevArray<uint32_t> tab(group * 2 * OL_ROW);
        DevArray<unsigned long long> best(group * n_asm), d_cursor(1), buf;
        if (want_sites) buf.alloc(cap);
        DevArray<unsigned long long> stable;
        ThermoScanArgs g{};                      // (a call without a model passes its ScanArgs part)
        g.tab = tab.p;
        g.lmin = lmin;
        g.max_mm = max_mm;
        g.n_asm = n_asm;
        g.n_sites = o.field[0].p;
        g.best = best.p;
        g.cursor = d_cursor.p;
        if (th) {
            stable.alloc(group * n_asm);
            g.model = model;
            g.max_dg = th->max_dg;
            g.n_stable = o.n_stable.p;
            g.stable = stable.p;
            if (want_sites) all_rows.alloc(nq * 2 * OL_ROW);
        }
        const StableFields sf{o.stable_sum[0].p, o.stable_sum[1].p, o.stable_sum[2].p, o.stable_at[0].p, o.stable_at[1].p, o.stable_at[2].p, o.stable_at[3].p};
        uint64_t rows = n_asm;
        for (uint64_t q0 = 0; q0 < nq; q0 += group, ++cnt.passes) {
            const uint64_t qn = std::min<uint64_t>(group, nq - q0);
            for (uint64_t q = 0; q < qn; ++q)
                pattern_rows(blob + offsets[q0 + q], (uint32_t)(offsets[q0 + q + 1] - offsets[q0 + q]), three_prime, rows_host.data() + q * 2 * OL_ROW);
            SW_HIP(hipMemcpyAsync(tab.p, rows_host.data(), qn * 2 * OL_ROW * 4, hipMemcpyHostToDevice, stream));
            SW_HIP(hipMemsetAsync(best.p, 0xFF, qn * n_asm * 8, stream));
            if (th) {
                SW_HIP(hipMemsetAsync(stable.p, 0xFF, qn * n_asm * 8, stream));
                if (want_sites) SW_HIP(hipMemcpyAsync(all_rows.p + q0 * 2 * OL_ROW, tab.p, qn * 2 * OL_ROW * 4, hipMemcpyDeviceToDevice, stream));
            }
            g.n_pat = (uint32_t)(2 * qn);
            g.q0 = (uint32_t)q0;
            for (uint64_t a0 = 0; a0 < n_asm;) {
                const uint64_t a1 = std::min<uint64_t>(n_asm, a0 + rows);
                SW_HIP(hipMemsetAsync(d_cursor.p, 0, 8, stream));
                g.buf = buf.p;
                g.cap = cap;
                g.v = runs.view(T.asm_tile_off[a0], T.asm_tile_off[a1]);
                cnt.launches += th ? launch_tiles(k_ol_scan<true>, g, blocks_max, stream) : launch_tiles(k_ol_scan<false>, (ScanArgs)g, blocks_max, stream);
                unsigned long long n = 0;
                SW_HIP(hipMemcpyAsync(&n, d_cursor.p, 8, hipMemcpyDeviceToHost, stream));
                SW_HIP(hipStreamSynchronize(stream));   // (the pattern rows of the host are free again, too)
                if (want_sites && n > cap) {
                    // the chunk's counts are partial: its columns of this pass's rows are cleared (the best sites are minima: a redo changes nothing)
                    SW_HIP(hipMemset2DAsync(o.field[0].p + q0 * n_asm + a0, n_asm * 4, 0, (a1 - a0) * 4, qn, stream));
                    if (th) {   // n_stable is as partial as n_sites; the stable keys go with it (minima, like the best sites: the redo finds them again)
                        SW_HIP(hipMemset2DAsync(o.n_stable.p + q0 * n_asm + a0, n_asm * 4, 0, (a1 - a0) * 4, qn, stream));
                        SW_HIP(hipMemset2DAsync(stable.p + a0, n_asm * 8, 0xFF, (a1 - a0) * 8, qn, stream));
                    }
                    overflow_step(a0, a1, rows, cap, buf, cnt);
                    continue;
                }
                cnt.hits += n;
                cnt.windows += T.asm_kmers[a1] - T.asm_kmers[a0];
                cnt.comparisons += (T.asm_kmers[a1] - T.asm_kmers[a0]) * 2 * qn;
                ++cnt.chunks;
                if (want_sites && n) {
                    if (cnt.hits >= OL_MAX_SITES) raise(SW_ERR_RUNTIME, "oligo hits: a site list of 2^32 entries or more");
                    lists.emplace_back((size_t)n);
                    SW_HIP(hipMemcpyAsync(lists.back().p, buf.p, n * 8, hipMemcpyDeviceToDevice, stream));
                }
                a0 = a1;
            }
            launch_1d(k_ol_resolve, qn * n_asm, stream, (const unsigned long long *)best.p, q0 * n_asm, runs.view(), o.field[1].p, o.field[2].p, o.field[3].p,
                      o.field[4].p);
            if (th) {
                SW_HIP(hipEventRecord(*ta, stream));
                launch_1d(k_ol_thermo_best, qn * n_asm, stream, (const unsigned long long *)stable.p, q0 * n_asm, runs.view(), (const uint32_t *)tab.p, n_asm, model, sf);
                SW_HIP(hipEventRecord(*tb, stream));
                SW_HIP(hipEventSynchronize(*tb));   // (the table is rewritten by the next pass)
                float t = 0;
                SW_HIP(hipEventElapsedTime(&t, *ta, *tb));
                best_ms += t;
            }
        }
    }
    SW_HIP(hipEventRecord(e1, stream));
    if (want_sites && cnt.hits) finish_site_list(lists, cnt.hits, k_ol_decode<OL_SITE_IDX_SHIFT, OL_SITE_Q_SHIFT - OL_SITE_IDX_SHIFT>, runs.view(), stream, o);
    SW_HIP(hipEventRecord(e2, stream));
    if (th && want_sites && cnt.hits) {
        for (int f = 0; f < 3; ++f) o.s_sum[f].alloc(cnt.hits);
        launch_1d(k_ol_thermo_sites, cnt.hits, stream, (const uint64_t *)o.keys.p, b.d_packed.p, (const uint32_t *)all_rows.p, model, o.s_sum[0].p, o.s_sum[1].p,
                  o.s_sum[2].p);
        SW_HIP(hipEventRecord(*tb, stream));
    }
    close_result(stream, e0, e1, e2, best_ms, cnt, o);
    o.thermo_ms[0] = best_ms;
    if (th && want_sites && cnt.hits) {
        float ms = 0;
        SW_HIP(hipEventElapsedTime(&ms, e2, *tb));
        o.thermo_ms[1] = ms;
    }
}

// ---- the route with indels ---------------------------------------------------------------------------------------------------------
// what max_edits adds to check_oligos
void check_edits(uint32_t lmin, uint64_t max_edits, uint64_t three_prime)
{
    if (max_edits > OLE_MAX_EDITS) raise(SW_ERR_VALUE, "oligo hits: max_edits must lie in 0..%u (got %llu)", OLE_MAX_EDITS, (unsigned long long)max_edits);
    if (max_edits + three_prime >= lmin)
        raise(SW_ERR_VALUE, "oligo hits: max_edits + three_prime must lie below the shortest oligo's %u letters (got %llu + %llu)", lmin,
              (unsigned long long)max_edits, (unsigned long long)three_prime);
}

// the row of oligo `text`: bit i of plane b is set iff base b lies in the set of position i; the length
void edit_row(const char *text, uint32_t len, uint32_t *row)
{
    memset(row, 0, ole::ROW * sizeof(uint32_t));
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t s = iupac_set((unsigned char)text[i]);
        for (uint32_t b = 0; b < 4; ++b)
            if ((s >> b) & 1) row[b] |= 1u << i;
    }
    row[4] = len;
}

// As batch_oligo_hits: groups of oligos, chunks of assemblies bounded by the buffer, halves and doublings on overflow, one sort.  The
// buffer holds the chunk's candidates whether or not the list is wanted: k_ole_resolve reads them.  Nothing is counted before a chunk
// is known to fit, so a chunk that is redone leaves nothing behind.
void batch_oligo_edit(const sw_batch &b, const uint64_t *offsets, const char *blob, uint64_t nq, uint32_t lmin, uint32_t d, uint32_t three_prime,
                      bool want_sites, hipStream_t stream, sw_oligos &o)
{
    const HostBatch &h = b.host;
    const uint64_t n_asm = h.n_assemblies, cells = nq * n_asm;
    start_result(b, offsets, nq, 0, d, three_prime, want_sites, 8, stream, o);
    const uint32_t k = lmin - d;   // a site spans L - d bases or more
    RunTiles T;
    build_run_tiles(h, k, "oligo hits", T);
    std::vector<uint64_t> asm_lanes(n_asm + 1, 0);   // lanes with an end, of the assemblies before a
    for (uint64_t r = 0; r < T.n_runs; ++r) asm_lanes[T.run_asm[r] + 1] += (T.run_nk[r] + KW_L - 1) / KW_L;
    for (uint64_t a = 0; a < n_asm; ++a) asm_lanes[a + 1] += asm_lanes[a];
    auto [group, cap, blocks_max] = chunk_sizes(nq);   // (cap doubles with the buffer)
    OligoCounts cnt;
    uint64_t steps = 0;
    double resolve_ms = 0;
    std::vector<DevArray<uint64_t>> lists;
    Event e0, e1, e2, ra, rb;
    SW_HIP(hipEventRecord(e0, stream));
    DevRunTiles runs(T, b.d_packed.p, stream, true);
    if (T.tiles && cells) {
        std::vector<uint32_t> rows_host(group * ole::ROW);
        DevArray<uint32_t> tab(group * ole::ROW);
        DevArray<unsigned long long> best(group * n_asm), d_cursor(1), buf(cap);
        EditScanArgs g{};
        g.tab = tab.p;
        g.k = k;
        g.d = d;
        g.c = three_prime;
        g.cursor = d_cursor.p;
        const BestFields bf{o.field[1].p, o.field[2].p, o.field[3].p, o.field[4].p, o.field[5].p, o.field[6].p, o.field[7].p};
        uint64_t rows = n_asm;
        for (uint64_t q0 = 0; q0 < nq; q0 += group, ++cnt.passes) {
            const uint64_t qn = std::min<uint64_t>(group, nq - q0);
            uint64_t len_sum = 0;
            for (uint64_t q = 0; q < qn; ++q) {
                edit_row(blob + offsets[q0 + q], o.lens[q0 + q], rows_host.data() + q * ole::ROW);
                len_sum += o.lens[q0 + q];
            }
            SW_HIP(hipMemcpyAsync(tab.p, rows_host.data(), qn * ole::ROW * 4, hipMemcpyHostToDevice, stream));
            SW_HIP(hipMemsetAsync(best.p, 0xFF, qn * n_asm * 8, stream));
            g.n_q = (uint32_t)qn;
            for (uint64_t a0 = 0; a0 < n_asm;) {
                const uint64_t a1 = std::min<uint64_t>(n_asm, a0 + rows);
                SW_HIP(hipMemsetAsync(d_cursor.p, 0, 8, stream));
                g.buf = buf.p;
                g.cap = cap;
                g.v = runs.view(T.asm_tile_off[a0], T.asm_tile_off[a1]);
                cnt.launches += launch_tiles(k_ole_scan, g, blocks_max, stream);
                unsigned long long n = 0;
                SW_HIP(hipMemcpyAsync(&n, d_cursor.p, 8, hipMemcpyDeviceToHost, stream));
                SW_HIP(hipStreamSynchronize(stream));   // (the rows of the host are free again, too)
                if (n > cap) {
                    overflow_step(a0, a1, rows, cap, buf, cnt);
                    continue;
                }
                const uint64_t ends = T.asm_kmers[a1] - T.asm_kmers[a0], lanes = asm_lanes[a1] - asm_lanes[a0];
                cnt.hits += n;
                cnt.windows += ends;
                cnt.comparisons += ends * 2 * qn;
                steps += 2 * (qn * ends + lanes * (len_sum + qn * 3 * d - qn));   // a lane steps L + 3 d - 1 bases more than it has ends
                ++cnt.chunks;
                if (n) {
                    if (want_sites && cnt.hits >= OL_MAX_SITES) raise(SW_ERR_RUNTIME, "oligo hits: a site list of 2^32 entries or more");
                    SW_HIP(hipEventRecord(ra, stream));
                    launch_1d(k_ole_resolve, n, stream, buf.p, (const uint32_t *)tab.p, (uint32_t)q0, runs.view(), k, d, three_prime, n_asm, o.field[0].p, best.p);
                    SW_HIP(hipEventRecord(rb, stream));
                    if (want_sites) {
                        lists.emplace_back((size_t)n);
                        SW_HIP(hipMemcpyAsync(lists.back().p, buf.p, n * 8, hipMemcpyDeviceToDevice, stream));
                    }
                    SW_HIP(hipEventSynchronize(rb));
                    float ms = 0;
                    SW_HIP(hipEventElapsedTime(&ms, ra, rb));
                    resolve_ms += ms;
                }
                a0 = a1;
            }
            launch_1d(k_ole_best, qn * n_asm, stream, (const unsigned long long *)best.p, q0 * n_asm, runs.view(), (const uint32_t *)tab.p, n_asm, d, bf);
            SW_HIP(hipStreamSynchronize(stream));   // (the table and the rows are rewritten by the next pass)
        }
    }
    SW_HIP(hipEventRecord(e1, stream));
    if (want_sites && cnt.hits) finish_site_list(lists, cnt.hits, k_ol_decode<OLE_IDX_SHIFT, OLE_SITE_Q_SHIFT - OLE_IDX_SHIFT>, runs.view(), stream, o);
    SW_HIP(hipEventRecord(e2, stream));
    close_result(stream, e0, e1, e2, resolve_ms, cnt, o);
    o.resolve_ms = resolve_ms;
    o.edit_counters[0] = steps;
    o.edit_counters[1] = cnt.hits;
}

}  // namespace
}  // namespace sw

using namespace sw;

extern "C" {

int sw_batch_oligo_hits(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_oligos, uint64_t max_mismatch, uint64_t three_prime,
                        int want_sites, void *stream, sw_oligos **out)
{
    return guarded([&] {
        const uint32_t lmin = check_oligos(offsets, blob, n_oligos, max_mismatch, three_prime);
        make_oligos(batch, stream, out, [&](sw_oligos &o) {
            batch_oligo_hits(*batch, offsets, blob, n_oligos, lmin, (uint32_t)max_mismatch, (uint32_t)three_prime, want_sites != 0, (hipStream_t)stream, o);
        });
    });
}

int sw_oligos_sizes(const sw_oligos *h, uint64_t *n_oligos, uint64_t *n_assemblies, uint64_t *max_mismatch, uint64_t *three_prime)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "oligo hits: a NULL handle");
        if (n_oligos) *n_oligos = h->nq;
        if (n_assemblies) *n_assemblies = h->n_asm;
        if (max_mismatch) *max_mismatch = h->max_mm;
        if (three_prime) *three_prime = h->three_prime;
    });
}

int sw_oligos_block(const sw_oligos *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "oligo hits: a NULL handle");
        if (field > 7)
            raise(SW_ERR_VALUE, "oligo hits: field %llu; 0 n_sites, 1 best_mm, 2 best_record, 3 best_pos, 4 best_strand, 5 best_end, 6 best_mismatch, 7 best_gaps",
                  (unsigned long long)field);
        // a Hamming result keeps no end, mismatch or gaps: they follow from pos + L, mm and 0
        const bool derived = field > 4 && h->max_edits < 0;
        const uint64_t src = !derived ? field : field == 5 ? 3 : 1;
        export_cells("oligo hits", "oligos", h->device, "the oligo hits", h->field[src].p, h->nq, h->n_asm, r0, r1, c0, c1, out);
        const uint64_t nr = r1 - r0, nc = c1 - c0;
        if (derived && field != 6)
            for (uint64_t r = 0; r < nr; ++r)
                for (uint64_t c = 0; c < nc; ++c)
                    if (out[r * nc + c] != 0xFFFFFFFFu) out[r * nc + c] = field == 5 ? out[r * nc + c] + h->lens[r0 + r] : 0;
    });
}

int sw_oligos_sites_size(const sw_oligos *h, uint64_t *n_sites_total)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "oligo hits: a NULL handle");
        if (!h->has_sites) raise(SW_ERR_VALUE, "oligo hits: these hits were made without the site list");
        if (n_sites_total) *n_sites_total = h->n_list;
    });
}

// the list's columns of either kind of result; dist (a Hamming result: mm), end, mismatch and gaps may each be NULL
static void site_columns(const sw_oligos *h, uint64_t *cell_offsets, uint32_t *oligo, uint32_t *assembly, uint32_t *record, uint32_t *pos, uint32_t *strand,
                         uint32_t *dist, uint32_t *end, uint32_t *mismatch, uint32_t *gaps)
{
    if (!h) raise(SW_ERR_VALUE, "oligo hits: a NULL handle");
    if (!h->has_sites) raise(SW_ERR_VALUE, "oligo hits: these hits were made without the site list");
    const uint64_t n = h->n_list, cells = h->nq * h->n_asm;
    if (!cell_offsets || (n && (!oligo || !assembly || !record || !pos || !strand))) raise(SW_ERR_VALUE, "oligo hits: a NULL handle or array");
    require_device(h->device, "the oligo hits");
    std::vector<uint32_t> counts(cells);
    if (cells) SW_HIP(hipMemcpy(counts.data(), h->field[0].p, cells * 4, hipMemcpyDeviceToHost));
    cell_offsets[0] = 0;
    for (uint64_t c = 0; c < cells; ++c) cell_offsets[c + 1] = cell_offsets[c] + counts[c];
    if (cell_offsets[cells] != n) raise(SW_ERR_RUNTIME, "internal error: the cells' site counts do not add up to the list");
    if (!n) return;
    std::vector<uint64_t> keys(n);
    SW_HIP(hipMemcpy(keys.data(), h->keys.p, n * 8, hipMemcpyDeviceToHost));
    SW_HIP(hipMemcpy(assembly, h->s_asm.p, n * 4, hipMemcpyDeviceToHost));
    SW_HIP(hipMemcpy(record, h->s_rec.p, n * 4, hipMemcpyDeviceToHost));
    SW_HIP(hipMemcpy(pos, h->s_pos.p, n * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t q, len_off, x, g;
        if (h->max_edits < 0) {
            q = (uint32_t)(keys[i] >> OL_SITE_Q_SHIFT);
            len_off = 0;
            x = (uint32_t)keys[i] & 15;
            g = 0;
        } else {
            const uint32_t d = (uint32_t)h->max_edits, over = (uint32_t)(keys[i] >> 5) & 15, code = (uint32_t)keys[i] & 15;
            q = (uint32_t)(keys[i] >> OLE_SITE_Q_SHIFT);
            len_off = over - d;   // (modulo 2^32: it is added to pos + L)
            x = code % 5;
            g = (over > d ? over - d : d - over) + 2 * (code / 5);
        }
        oligo[i] = q;
        strand[i] = (uint32_t)(keys[i] >> 4) & 1;
        if (dist) dist[i] = x + g;
        if (end) end[i] = pos[i] + h->lens[q] + len_off;
        if (mismatch) mismatch[i] = x;
        if (gaps) gaps[i] = g;
    }
}

int sw_oligos_sites(const sw_oligos *h, uint64_t *cell_offsets, uint32_t *oligo, uint32_t *assembly, uint32_t *record, uint32_t *pos, uint32_t *strand,
                    uint32_t *mm)
{
    return guarded([&] {
        if (h && h->n_list && !mm) raise(SW_ERR_VALUE, "oligo hits: a NULL handle or array");
        site_columns(h, cell_offsets, oligo, assembly, record, pos, strand, mm, nullptr, nullptr, nullptr);
    });
}

int sw_oligos_sites_edit(const sw_oligos *h, uint64_t *cell_offsets, uint32_t *oligo, uint32_t *assembly, uint32_t *record, uint32_t *pos, uint32_t *strand,
                         uint32_t *end, uint32_t *mismatch, uint32_t *gaps)
{
    return guarded([&] {
        if (h && h->n_list && (!end || !mismatch || !gaps)) raise(SW_ERR_VALUE, "oligo hits: a NULL handle or array");
        site_columns(h, cell_offsets, oligo, assembly, record, pos, strand, nullptr, end, mismatch, gaps);
    });
}

int sw_batch_oligo_hits_edit(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_oligos, uint64_t max_edits, uint64_t three_prime,
                             int want_sites, void *stream, sw_oligos **out)
{
    return guarded([&] {
        const uint32_t lmin = check_oligos(offsets, blob, n_oligos, 0, three_prime);
        check_edits(lmin, max_edits, three_prime);
        make_oligos(batch, stream, out, [&](sw_oligos &o) {
            batch_oligo_edit(*batch, offsets, blob, n_oligos, lmin, (uint32_t)max_edits, (uint32_t)three_prime, want_sites != 0, (hipStream_t)stream, o);
        });
    });
}

int sw_oligos_max_edits(const sw_oligos *h, int64_t *max_edits)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "oligo hits: a NULL handle");
        if (max_edits) *max_edits = h->max_edits;
    });
}

int sw_oligos_edit_stats(const sw_oligos *h, uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "oligo hits: a NULL handle");
        if (counters) memcpy(counters, h->edit_counters, sizeof h->edit_counters);
        if (ms) *ms = h->resolve_ms;
    });
}

int sw_oligos_stats(const sw_oligos *h, uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "oligo hits: a NULL handle");
        if (counters) memcpy(counters, h->counters, sizeof h->counters);
        if (ms) memcpy(ms, h->ms, sizeof h->ms);
    });
}

int sw_batch_oligo_hits_thermo(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_oligos, uint64_t max_mismatch, uint64_t three_prime,
                               int want_sites, void *stream, const int16_t *stack, const int16_t *end, const int32_t *init, int64_t max_dg, int no_threshold,
                               sw_oligos **out)
{
    return guarded([&] {
        const uint32_t lmin = check_oligos(offsets, blob, n_oligos, max_mismatch, three_prime);
        const ThermoModel th{stack, end, init, no_threshold ? INT32_MAX : (int32_t)std::min<int64_t>(std::max<int64_t>(max_dg, INT32_MIN), INT32_MAX)};
        check_model(th);
        make_oligos(batch, stream, out, [&](sw_oligos &o) {
            batch_oligo_hits(*batch, offsets, blob, n_oligos, lmin, (uint32_t)max_mismatch, (uint32_t)three_prime, want_sites != 0, (hipStream_t)stream, o, &th);
        });
    });
}

int sw_oligos_thermo_block(const sw_oligos *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, void *out)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "oligo hits: a NULL handle");
        if (!h->thermo) raise(SW_ERR_VALUE, "oligo hits: these hits were made without a thermodynamic model");
        if (field > 7)
            raise(SW_ERR_VALUE, "oligo hits: thermo field %llu; 0 n_stable, 1 stable_dg, 2 stable_dh, 3 stable_ds, 4 stable_record, 5 stable_pos, 6 stable_strand, 7 stable_mm",
                  (unsigned long long)field);
        const void *src = field == 0 ? (const void *)h->n_stable.p : field < 4 ? (const void *)h->stable_sum[field - 1].p : (const void *)h->stable_at[field - 4].p;
        export_cells("oligo hits", "oligos", h->device, "the oligo hits", src, h->nq, h->n_asm, r0, r1, c0, c1, out);
    });
}

int sw_oligos_sites_thermo(const sw_oligos *h, int32_t *dh, int32_t *ds, int32_t *dg)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "oligo hits: a NULL handle");
        if (!h->thermo) raise(SW_ERR_VALUE, "oligo hits: these hits were made without a thermodynamic model");
        if (!h->has_sites) raise(SW_ERR_VALUE, "oligo hits: these hits were made without the site list");
        if (!h->n_list) return;
        if (!dh || !ds || !dg) raise(SW_ERR_VALUE, "oligo hits: a NULL handle or array");
        require_device(h->device, "the oligo hits");
        int32_t *dst[3] = {dh, ds, dg};
        for (int f = 0; f < 3; ++f) SW_HIP(hipMemcpy(dst[f], h->s_sum[f].p, h->n_list * 4, hipMemcpyDeviceToHost));
    });
}

int sw_oligos_thermo_stats(const sw_oligos *h, uint64_t *stable_hits, double *ms)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "oligo hits: a NULL handle");
        if (!h->thermo) raise(SW_ERR_VALUE, "oligo hits: these hits were made without a thermodynamic model");
        if (stable_hits) {   // summed when asked for: the search itself never reads n_stable back
            const uint64_t cells = h->nq * h->n_asm;
            std::vector<uint32_t> n(cells);
            if (cells) {
                require_device(h->device, "the oligo hits");
                SW_HIP(hipMemcpy(n.data(), h->n_stable.p, cells * 4, hipMemcpyDeviceToHost));
            }
            *stable_hits = 0;
            for (uint32_t x : n) *stable_hits += x;
        }
        if (ms) memcpy(ms, h->thermo_ms, sizeof h->thermo_ms);
    });
}

void sw_oligos_free(sw_oligos *h)
{
    delete h;
}

}  // extern "C"
