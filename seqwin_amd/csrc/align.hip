// align.hip -- the canonical optimal alignment behind the infix edit distance of hits.hip: where the located copy starts, how the
// distance splits into mismatches and gaps, and on request the edit script.
//
// No counterpart in the reference: NOT BLAST, no scores, no e-values, no local alignment, none of MarkerMetrics.  DESIGN.md section
// 3.2f is the specification; tests/tools/align_host.py restates it.
//
// Layer A (hits.hip) ran first and gave dist and j* (end - start) of a pair.  The canonical path costs dist, so it has at most dist
// gaps: it stays on the diagonals j - i of [j* - m - dist, j* - m + dist] and in the columns [max(0, j* - m - dist), j*].
//   k_al_size    the band's geometry per pair: cells of scratch, the class of the store launch that takes it
//   k_al_store   Layer A's block recurrence once more from column 0 of the window to column j*; every (block, column) cell the band
//                touches keeps Pv, Mv (the vertical deltas of the column) and the score of the block's bottom row.  One strand, the
//                register route in groups of 2^c lanes; k_al_store_striped: queries above the block bound, with the HBM carry row
//   k_al_walk    one lane per pair, rules 1-4 of the specification on the stored cells.  Rule 2 asks D[i-1][j-1], which is the bottom
//                score of its cell minus the vertical deltas below the row; rule 3 is bit i-1 of Pv at (i, j); rule 4 is what is left
//   k_al_compact the scripts out of their padded slots into CSR
// Pairs go through the scratch in rounds of at most the budget; a pair above it gets a round and a scratch of its own.
#include "hits_core.hpp"

namespace sw {
namespace {

constexpr uint64_t ALN_SCRATCH_BYTES = 1ull << 30;   // Pv, Mv and bottom scores of one round: speed only, no measurement behind it
constexpr uint64_t ALN_CELL_BYTES = 20;              // two 64-bit planes and a 32-bit score
constexpr uint32_t ALN_NO_CLASS = 0xFF;

// The band of a pair with m >= 1 rows whose best column is js >= 1 at distance dist (<= m).
struct Band {
    long long khi;    // the largest diagonal j - i the path can reach
    uint64_t cmin;    // columns cmin + 1 .. js are stored
    uint32_t W;       // blocks kept per column
};

__host__ __device__ inline Band band_of(uint32_t m, uint32_t js, uint32_t dist)
{
    Band b;
    const long long klo = (long long)js - m - (long long)dist;
    b.khi = (long long)js - m + (long long)dist;
    b.cmin = klo > 0 ? (uint64_t)klo : 0;
    const uint64_t nb = ((uint64_t)m + 63) >> 6, w = (2ull * dist + 1 + 63) / 64 + 1;
    b.W = (uint32_t)(w < nb ? w : nb);
    return b;
}

// the first block kept of column j: the block of row max(1, j - khi)
__device__ __forceinline__ uint32_t band_first_block(const Band &b, uint32_t j)
{
    const long long r = (long long)j - b.khi;
    return r > 1 ? (uint32_t)((r - 1) >> 6) : 0u;
}

// index of cell (block B, column j) in the pair's scratch, or ~0 if the band does not hold it
__device__ __forceinline__ uint64_t band_slot(const Band &b, uint32_t B, uint32_t j)
{
    if (j <= b.cmin) return ~0ull;
    const uint32_t b0 = band_first_block(b, j);
    if (B < b0 || B - b0 >= b.W) return ~0ull;
    return ((uint64_t)j - b.cmin - 1) * b.W + (B - b0);
}

struct AlArgs {
    RunTable t;
    const uint32_t *codes[2], *valid[2];
    const uint64_t *qoff;
    const sw_infix_pair *pairs;
    const uint32_t *out_idx;      // where pair i's results lie and go (nullptr: i)
    const uint32_t *dist, *end;   // Layer A's results
    const uint64_t *cell_off;     // [n + 1] prefix sums of the pairs' cells
    uint64_t round_base;          // cell_off of the round's first pair
    uint64_t *pv, *mv;            // the round's scratch
    uint32_t *sc;
    const uint32_t *list;         // store: pair indices of this launch's class
    uint64_t count;
    uint32_t g;                   // store: lanes per pair (a power of two <= 64)
    uint8_t *carry;               // striped route: one row of carry_stride bytes per group of the launch
    uint64_t carry_stride;
    uint32_t *a_start, *nident, *mismatch, *gaps;
    uint8_t *ops;                 // nullptr: no scripts
    const uint64_t *ops_end;
    uint32_t *fail;               // set by a walk that left its band or its slot: an internal error, nothing is read or written outside
};

// cells of every pair and the class of its store launch (ALN_NO_CLASS: nothing to store -- an empty side or j* = 0)
// stat[0]: longest text prefix (j*) of the striped class
__global__ __launch_bounds__(SQ_TPB) void k_al_size(const sw_infix_pair *__restrict__ pairs, const uint32_t *__restrict__ out_idx, const uint64_t *__restrict__ qoff,
                                                    const uint32_t *__restrict__ dist, const uint32_t *__restrict__ end, uint64_t n, uint32_t cap,
                                                    uint64_t *__restrict__ cells, uint8_t *__restrict__ cls, unsigned long long *__restrict__ stat)
{
    const uint64_t i = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x;
    if (i >= n) return;
    const sw_infix_pair p = pairs[i];
    const uint32_t oi = out_idx ? out_idx[i] : (uint32_t)i;
    const uint32_t m = (uint32_t)(qoff[p.query + 1] - qoff[p.query]), js = end[oi] - p.start;
    uint64_t c = 0;
    uint32_t k = ALN_NO_CLASS;
    if (m && js) {
        const Band b = band_of(m, js, dist[oi]);
        c = ((uint64_t)js - b.cmin) * b.W;
        const uint32_t nb = (m + 63) >> 6;
        k = 0;
        if (nb > cap) {
            k = ED_CLASSES - 1;
            atomicMax(stat, (unsigned long long)js);
        } else
            while ((1u << k) < nb) ++k;
    }
    cells[i] = c;
    cls[i] = (uint8_t)k;
}

// The group's lanes call this together: infix_pair (hits.hip) over columns 1 .. j* of the window, keeping the band's cells.
__device__ void store_pair(const AlArgs &a, uint32_t i, uint32_t g, uint32_t b, uint8_t *carry)
{
    const RunTable &t = a.t;
    const sw_infix_pair p = a.pairs[i];
    const uint32_t oi = a.out_idx ? a.out_idx[i] : i;
    const uint64_t qbase = a.qoff[p.query];
    const uint32_t m = (uint32_t)(a.qoff[p.query + 1] - qbase), n = a.end[oi] - p.start;   // columns 1 .. j*
    const Band band = band_of(m, n, a.dist[oi]);
    const uint64_t base = a.cell_off[i] - a.round_base;
    const uint32_t *codes = a.codes[p.strand & 1u], *valid = a.valid[p.strand & 1u];
    const uint32_t nb = (m + 63) >> 6, n_stripes = (nb + g - 1) / g;
    const uint64_t tbase = t.rec_base[p.record] + p.start;
    RunMemo tm;
    for (uint32_t s = 0; s < n_stripes; ++s) {
        const uint32_t B = s * g + b, sb = nb - s * g < g ? nb - s * g : g;
        const bool active = b < sb, last_block = B == nb - 1, first = s == 0;
        const bool leaves_carry = active && b == sb - 1 && !last_block;
        uint64_t lo = 0, hi = 0, vm = 0;
        if (active) {
            const uint32_t pos = 64 * B, cnt = m - pos < 64 ? m - pos : 64, c0 = cnt < 32 ? cnt : 32, c1 = cnt - c0;
            const uint64_t x0 = load_codes(codes, qbase + pos, c0);
            vm = plane32(valid, qbase + pos, c0);
            lo = even_bits(x0);
            hi = even_bits(x0 >> 1);
            if (c1) {
                const uint64_t x1 = load_codes(codes, qbase + pos + 32, c1);
                vm |= (uint64_t)plane32(valid, qbase + pos + 32, c1) << 32;
                lo |= (uint64_t)even_bits(x1) << 32;
                hi |= (uint64_t)even_bits(x1 >> 1) << 32;
            }
        }
        const uint32_t out_bit = last_block ? (m - 1) & 63u : 63u;
        uint32_t score = last_block ? m : 64 * (B + 1);   // D of the block's bottom row in column 0
        uint64_t Pv = ~0ull, Mv = 0;
        uint64_t tf = 0, cbuf = 0;
        uint32_t vf = 0;
        uint32_t msg = 0;
        const uint32_t steps = n + sb - 1;
        for (uint32_t step = 0; step < steps; ++step) {
            uint32_t in = __shfl_up(msg, 1, g);
            if (b == 0 && step < n) {
                const uint32_t x = step & 31u;
                if (x == 0) {
                    const uint32_t cnt = n - step < 32 ? n - step : 32;
                    tf = load_codes(t.packed, tbase + step, cnt);
                    vf = valid32(t, p.record, p.start + step, cnt, tm);
                }
                const uint32_t cf = ((vf >> x) & 1u) ? (uint32_t)(tf >> (2 * x)) & 3u : 4u;
                uint32_t hf = 0;
                if (!first) {
                    if ((step & 7u) == 0) cbuf = *reinterpret_cast<const uint64_t *>(carry + step);
                    hf = (uint32_t)(cbuf >> (8 * (step & 7u))) & 3u;
                }
                in = cf | (hf << 3);
            }
            const uint32_t col = step - b;   // (wraps below zero: then >= n)
            if (active && step >= b && col < n) {
                const uint32_t cf = in & 7u, hf = (in >> 3) & 3u;
                const uint64_t ef = cf < 4 ? ~(lo ^ (0ull - (cf & 1u))) & ~(hi ^ (0ull - ((cf >> 1) & 1u))) & vm : 0ull;
                const uint32_t of = myers_step(ef, Pv, Mv, hf, out_bit);
                score += of == 1 ? 1u : of == 2 ? 0xFFFFFFFFu : 0u;
                const uint64_t slot = band_slot(band, B, col + 1);
                if (slot != ~0ull) {
                    a.pv[base + slot] = Pv;
                    a.mv[base + slot] = Mv;
                    a.sc[base + slot] = score;
                }
                if (leaves_carry) carry[col] = (uint8_t)of;
                msg = cf | (of << 3);
            }
        }
        if (n_stripes > 1) __threadfence();   // the row is complete and visible before the next stripe reads it
    }
}

__global__ __launch_bounds__(SQ_TPB) void k_al_store(AlArgs a)
{
    const uint64_t tid = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x, grp = tid / a.g;
    if (grp >= a.count) return;   // (whole groups)
    store_pair(a, a.list[grp], a.g, (uint32_t)(tid % a.g), nullptr);
}

__global__ __launch_bounds__(SQ_TPB) void k_al_store_striped(AlArgs a, uint32_t groups)
{
    const uint64_t tid = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x, grp = tid / a.g;
    if (grp >= groups) return;
    for (uint64_t x = grp; x < a.count; x += groups) {
        store_pair(a, a.list[x], a.g, (uint32_t)(tid % a.g), a.carry + grp * a.carry_stride);
        __threadfence();   // (the row is reused by the group's next pair)
    }
}

// pairs [p0, p1) of the list, one lane each
__global__ __launch_bounds__(SQ_TPB) void k_al_walk(AlArgs a, uint64_t p0, uint64_t p1)
{
    const uint64_t i = p0 + (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x;
    if (i >= p1) return;
    const RunTable &t = a.t;
    const sw_infix_pair p = a.pairs[i];
    const uint32_t oi = a.out_idx ? a.out_idx[i] : (uint32_t)i;
    const uint64_t qbase = a.qoff[p.query];
    const uint32_t m = (uint32_t)(a.qoff[p.query + 1] - qbase), js = a.end[oi] - p.start;
    const uint32_t *codes = a.codes[p.strand & 1u], *valid = a.valid[p.strand & 1u];
    const uint64_t tbase = t.rec_base[p.record] + p.start;
    const uint32_t nb = (m + 63) >> 6;
    uint32_t d = a.dist[oi];
    Band band{};
    if (m && js) band = band_of(m, js, d);
    const uint64_t base = a.cell_off[i] - a.round_base;
    uint64_t w = a.ops ? a.ops_end[i] : 0;
    RunMemo tm;
    uint32_t ni = 0, nx = 0, ng = 0, r = m, j = js;
    uint64_t room = (uint64_t)m + d;   // ops a path of cost dist has at most
    while (r > 0) {
        if (room-- == 0) {
            atomicOr(a.fail, 1u);
            break;
        }
        uint32_t op = 2;   // column 0: D[r][0] = r, only rule 3 is left
        if (j > 0) {
            const uint64_t qx = qbase + r - 1;
            const bool pvalid = (valid[qx >> 5] >> (qx & 31)) & 1u;
            const uint32_t pc = (uint32_t)load_codes(codes, qx, 1) & 3u;
            const bool tvalid = valid32(t, p.record, p.start + j - 1, 1, tm) & 1u;
            const uint32_t tc = (uint32_t)load_codes(t.packed, tbase + j - 1, 1) & 3u;
            if (pvalid && tvalid && pc == tc) {
                op = 0;
            } else {
                // D[r - 1][j - 1]: 0 in row 0, the row in column 0, else the bottom score of its cell minus the deltas below the row
                uint32_t diag;
                if (r == 1) diag = 0;
                else if (j == 1) diag = r - 1;
                else {
                    const uint32_t B = (r - 2) >> 6, bit = (r - 2) & 63u, ob = B == nb - 1 ? (m - 1) & 63u : 63u;
                    const uint64_t slot = band_slot(band, B, j - 1);
                    if (slot == ~0ull) {
                        atomicOr(a.fail, 1u);
                        break;
                    }
                    const uint64_t at = base + slot;
                    const uint64_t below = (ob == 63 ? ~0ull : (1ull << (ob + 1)) - 1) & ~((2ull << bit) - 1);   // rows bit + 1 .. ob
                    diag = a.sc[at] - (uint32_t)__popcll(a.pv[at] & below) + (uint32_t)__popcll(a.mv[at] & below);
                }
                if (diag + 1 == d) op = 1;
                else {
                    const uint64_t slot = band_slot(band, (r - 1) >> 6, j);
                    if (slot == ~0ull) {
                        atomicOr(a.fail, 1u);
                        break;
                    }
                    const uint64_t at = base + slot;
                    op = ((a.pv[at] >> ((r - 1) & 63u)) & 1ull) ? 2 : 3;
                }
            }
        }
        if (op == 0) ++ni;
        else if (op == 1) ++nx;
        else ++ng;
        if (op != 0) --d;
        if (op != 3) --r;
        if (op != 2) --j;
        if (a.ops) a.ops[--w] = (uint8_t)op;
    }
    a.a_start[oi] = p.start + j;
    a.nident[oi] = ni;
    a.mismatch[oi] = nx;
    a.gaps[oi] = ng;
}

// The pile form of the walk: k_al_walk's rules on the same cells, the same four figures, and every column of
// a piled pair added to the sink as it is decided.  The walk runs backwards: rules 1-3 consume pattern index r - 1, which is query
// position r - 1 on strand 0 and m - r on strand 1; a run of rule 4 stays in a register and goes to its slot -- r on strand 0, m - r
// on strand 1 -- when the next other op closes it.  Every add is an integer atomic whose result nobody reads.
__device__ void pile_pair(const AlArgs &a, const PileSink &s, uint64_t i, unsigned long long *tally)
{
    const RunTable &t = a.t;
    const sw_infix_pair p = a.pairs[i];
    const uint32_t oi = a.out_idx ? a.out_idx[i] : (uint32_t)i;
    const uint64_t qbase = a.qoff[p.query];
    const uint32_t m = (uint32_t)(a.qoff[p.query + 1] - qbase), js = a.end[oi] - p.start;
    const uint32_t strand = p.strand & 1u;
    const uint32_t *codes = a.codes[strand], *valid = a.valid[strand];
    const uint64_t tbase = t.rec_base[p.record] + p.start;
    const uint32_t nb = (m + 63) >> 6;
    uint32_t d = a.dist[oi];
    // labels were checked on the host: below n_groups, or PILE_LEAVE_OUT
    const uint32_t lab = s.group[s.group_mod ? oi % s.group_mod : oi];
    const bool labelled = lab < s.n_groups, piled = labelled && (uint64_t)d * 1000 <= (uint64_t)s.max_dist_permille * m;
    const uint64_t stride = (uint64_t)s.n_groups * PILE_CLASSES;
    uint32_t *const rows = s.table + qbase * stride + (piled ? lab : 0u) * PILE_CLASSES;   // class c of position u: rows[u * stride + c]
    Band band{};
    if (m && js) band = band_of(m, js, d);
    const uint64_t base = a.cell_off[i] - a.round_base;
    RunMemo tm;
    uint32_t ni = 0, nx = 0, ng = 0, r = m, j = js, run = 0, adds = 0;
    uint64_t room = (uint64_t)m + d;   // ops a path of cost dist has at most
    while (r > 0) {
        if (room-- == 0) {
            atomicOr(a.fail, 1u);
            break;
        }
        uint32_t op = 2;   // column 0: D[r][0] = r, only rule 3 is left
        uint32_t tcls = 4; // the class of text base j - 1 in the query's orientation
        if (j > 0) {
            const uint64_t qx = qbase + r - 1;
            const bool pvalid = (valid[qx >> 5] >> (qx & 31)) & 1u;
            const uint32_t pc = (uint32_t)load_codes(codes, qx, 1) & 3u;
            const bool tvalid = valid32(t, p.record, p.start + j - 1, 1, tm) & 1u;
            const uint32_t tc = (uint32_t)load_codes(t.packed, tbase + j - 1, 1) & 3u;
            if (tvalid) tcls = strand ? 3u - tc : tc;
            if (pvalid && tvalid && pc == tc) {
                op = 0;
            } else {
                uint32_t diag;
                if (r == 1) diag = 0;
                else if (j == 1) diag = r - 1;
                else {
                    const uint32_t B = (r - 2) >> 6, bit = (r - 2) & 63u, ob = B == nb - 1 ? (m - 1) & 63u : 63u;
                    const uint64_t slot = band_slot(band, B, j - 1);
                    if (slot == ~0ull) {
                        atomicOr(a.fail, 1u);
                        break;
                    }
                    const uint64_t at = base + slot;
                    const uint64_t below = (ob == 63 ? ~0ull : (1ull << (ob + 1)) - 1) & ~((2ull << bit) - 1);   // rows bit + 1 .. ob
                    diag = a.sc[at] - (uint32_t)__popcll(a.pv[at] & below) + (uint32_t)__popcll(a.mv[at] & below);
                }
                if (diag + 1 == d) op = 1;
                else {
                    const uint64_t slot = band_slot(band, (r - 1) >> 6, j);
                    if (slot == ~0ull) {
                        atomicOr(a.fail, 1u);
                        break;
                    }
                    const uint64_t at = base + slot;
                    op = ((a.pv[at] >> ((r - 1) & 63u)) & 1ull) ? 2 : 3;
                }
            }
        }
        if (piled) {
            if (op == 3) ++run;
            else {
                if (run) {
                    // the run lies before pattern index r, which is neither 0 (the walk would have stopped) nor m (j* is the smallest
                    // column of the minimum): its slot lies inside the query's rows
                    if (r >= m) {
                        atomicOr(a.fail, 1u);
                        break;
                    }
                    uint32_t *const slot = rows + (uint64_t)(strand ? m - r : r) * stride;
                    atomicAdd(slot + 6, 1u);
                    atomicAdd(slot + 7, run);
                    adds += 2;
                    run = 0;
                }
                atomicAdd(rows + (uint64_t)(strand ? m - r : r - 1) * stride + (op == 2 ? 5u : tcls), 1u);
                ++adds;
            }
        }
        if (op == 0) ++ni;
        else if (op == 1) ++nx;
        else ++ng;
        if (op != 0) --d;
        if (op != 3) --r;
        if (op != 2) --j;
    }
    if (run) atomicOr(a.fail, 1u);   // (a script does not begin with D)
    a.a_start[oi] = p.start + j;
    a.nident[oi] = ni;
    a.mismatch[oi] = nx;
    a.gaps[oi] = ng;
    if (piled) {
        atomicAdd(s.depth + (uint64_t)p.query * s.n_groups + lab, 1u);
        atomicAdd(tally + PS_ADDS, (unsigned long long)adds);
    }
    atomicAdd(tally + (piled ? PS_PILED : labelled ? PS_FILTERED : PS_LEFT_OUT), 1ull);
}

// pairs [p0, p1) of the list, one lane each; the workgroup's counters go to the sink's in one add each
__global__ __launch_bounds__(SQ_TPB) void k_al_walk_pile(AlArgs a, PileSink s, uint64_t p0, uint64_t p1)
{
    __shared__ unsigned long long tally[PS_N];
    if (threadIdx.x < PS_N) tally[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = p0 + (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x;
    if (i < p1) pile_pair(a, s, i, tally);
    __syncthreads();
    if (threadIdx.x < PS_N && tally[threadIdx.x]) atomicAdd(s.stat + threadIdx.x, tally[threadIdx.x]);
}

// The window form of the walk: pile_pair's rules, figures and adds, written out again so that the pile walk
// keeps its code, plus the class of every window of the sink's lengths.  The walk runs backwards, so three shift registers stand in
// for the script: after pattern index s = r - 1 is consumed, bit t of X / INS says that the column consuming index s + t is `X` / `I`,
// and bit t of B that a run of `D` lies before index s + t (a closed run sets bit 0 before the next shift).  With m - s >= L the
// window [s, s + L) is complete: e = popc(X & maskL); it is gapped iff (INS & maskL) | (B & maskL & ~1) -- a run before index s or
// s + L lies at the window's edge and does not gap it.  The window's row is u = s on strand 0 and m - L - s on strand 1, where the
// two tails change ends.  Only an imperfect window adds here (classes 1..5, and 6 / 7 where they hold): k_win_finish fills MM0 from
// the depth and adds it to FWD_OK and REV_OK.  Every add is an integer atomic whose result nobody reads.
__device__ void win_pair(const AlArgs &a, const PileSink &s, const WinSink &ws, uint64_t i, unsigned long long *tally, unsigned long long *wtally)
{
    const RunTable &t = a.t;
    const sw_infix_pair p = a.pairs[i];
    const uint32_t oi = a.out_idx ? a.out_idx[i] : (uint32_t)i;
    const uint64_t qbase = a.qoff[p.query];
    const uint32_t m = (uint32_t)(a.qoff[p.query + 1] - qbase), js = a.end[oi] - p.start;
    const uint32_t strand = p.strand & 1u;
    const uint32_t *codes = a.codes[strand], *valid = a.valid[strand];
    const uint64_t tbase = t.rec_base[p.record] + p.start;
    const uint32_t nb = (m + 63) >> 6;
    uint32_t d = a.dist[oi];
    // labels were checked on the host: below n_groups, or PILE_LEAVE_OUT
    const uint32_t lab = s.group[s.group_mod ? oi % s.group_mod : oi];
    const bool labelled = lab < s.n_groups, piled = labelled && (uint64_t)d * 1000 <= (uint64_t)s.max_dist_permille * m;
    const uint64_t stride = (uint64_t)s.n_groups * PILE_CLASSES;
    uint32_t *const rows = s.table + qbase * stride + (piled ? lab : 0u) * PILE_CLASSES;   // class c of position u: rows[u * stride + c]
    const uint64_t wstride = (uint64_t)ws.n_lengths * s.n_groups * WIN_CLASSES, lstride = (uint64_t)s.n_groups * WIN_CLASSES;
    uint32_t *const wrows = ws.table + qbase * wstride + (piled ? lab : 0u) * WIN_CLASSES;   // class c of window u, length l: wrows[u * wstride + l * lstride + c]
    const uint32_t c3 = ws.three_prime, tail = c3 ? (1u << c3) - 1 : 0u;   // (three_prime <= 8 <= every length)
    Band band{};
    if (m && js) band = band_of(m, js, d);
    const uint64_t base = a.cell_off[i] - a.round_base;
    RunMemo tm;
    uint32_t ni = 0, nx = 0, ng = 0, r = m, j = js, run = 0, adds = 0, wadds = 0, seen = 0;
    uint32_t X = 0, INS = 0, B = 0;
    uint64_t room = (uint64_t)m + d;   // ops a path of cost dist has at most
    while (r > 0) {
        if (room-- == 0) {
            atomicOr(a.fail, 1u);
            break;
        }
        uint32_t op = 2;   // column 0: D[r][0] = r, only rule 3 is left
        uint32_t tcls = 4; // the class of text base j - 1 in the query's orientation
        if (j > 0) {
            const uint64_t qx = qbase + r - 1;
            const bool pvalid = (valid[qx >> 5] >> (qx & 31)) & 1u;
            const uint32_t pc = (uint32_t)load_codes(codes, qx, 1) & 3u;
            const bool tvalid = valid32(t, p.record, p.start + j - 1, 1, tm) & 1u;
            const uint32_t tc = (uint32_t)load_codes(t.packed, tbase + j - 1, 1) & 3u;
            if (tvalid) tcls = strand ? 3u - tc : tc;
            if (pvalid && tvalid && pc == tc) {
                op = 0;
            } else {
                uint32_t diag;
                if (r == 1) diag = 0;
                else if (j == 1) diag = r - 1;
                else {
                    const uint32_t Bk = (r - 2) >> 6, bit = (r - 2) & 63u, ob = Bk == nb - 1 ? (m - 1) & 63u : 63u;
                    const uint64_t slot = band_slot(band, Bk, j - 1);
                    if (slot == ~0ull) {
                        atomicOr(a.fail, 1u);
                        break;
                    }
                    const uint64_t at = base + slot;
                    const uint64_t below = (ob == 63 ? ~0ull : (1ull << (ob + 1)) - 1) & ~((2ull << bit) - 1);   // rows bit + 1 .. ob
                    diag = a.sc[at] - (uint32_t)__popcll(a.pv[at] & below) + (uint32_t)__popcll(a.mv[at] & below);
                }
                if (diag + 1 == d) op = 1;
                else {
                    const uint64_t slot = band_slot(band, (r - 1) >> 6, j);
                    if (slot == ~0ull) {
                        atomicOr(a.fail, 1u);
                        break;
                    }
                    const uint64_t at = base + slot;
                    op = ((a.pv[at] >> ((r - 1) & 63u)) & 1ull) ? 2 : 3;
                }
            }
        }
        if (piled) {
            if (op == 3) ++run;
            else {
                if (run) {
                    // the run lies before pattern index r, which is neither 0 (the walk would have stopped) nor m (j* is the smallest
                    // column of the minimum): its slot lies inside the query's rows
                    if (r >= m) {
                        atomicOr(a.fail, 1u);
                        break;
                    }
                    uint32_t *const slot = rows + (uint64_t)(strand ? m - r : r) * stride;
                    atomicAdd(slot + 6, 1u);
                    atomicAdd(slot + 7, run);
                    adds += 2;
                    run = 0;
                    B |= 1u;   // bit 0 is still index r, the last one consumed
                }
                atomicAdd(rows + (uint64_t)(strand ? m - r : r - 1) * stride + (op == 2 ? 5u : tcls), 1u);
                ++adds;
                // index r - 1 is consumed: it becomes bit 0
                X = (X << 1) | (op == 1 ? 1u : 0u);
                INS = (INS << 1) | (op == 2 ? 1u : 0u);
                B <<= 1;
                const uint32_t ws0 = r - 1, left = m - ws0;   // the pattern indices from ws0 on
                for (uint32_t l = 0; l < ws.n_lengths; ++l) {
                    const uint32_t L = ws.len[l];
                    if (left < L) continue;
                    ++seen;
                    const uint32_t mask = L >= 32 ? ~0u : (1u << L) - 1;
                    const uint32_t xm = X & mask;
                    // (B was shifted just above, so its bit 0 is 0 here and `& ~1u` removes nothing: it stands as section 3.2l words the test)
                    const bool gapped = ((INS & mask) | (B & mask & ~1u)) != 0;
                    if (!gapped && !xm) continue;   // a perfect window: the finishing pass counts it
                    const uint32_t u = strand ? left - L : ws0;   // u + L <= m by left >= L
                    if ((uint64_t)u + L > m) {
                        atomicOr(a.fail, 1u);
                        continue;
                    }
                    uint32_t *const slot = wrows + (uint64_t)u * wstride + (uint64_t)l * lstride;
                    if (gapped) {
                        atomicAdd(slot + 5, 1u);
                        ++wadds;
                        continue;
                    }
                    const uint32_t e = (uint32_t)__popc(xm);
                    atomicAdd(slot + (e < 4 ? e : 4u), 1u);
                    ++wadds;
                    if (e <= ws.max_mismatch) {
                        // pattern indices rise with the query's positions on strand 0 and fall with them on strand 1
                        const bool low_bad = (xm & tail) != 0, high_bad = c3 && ((xm >> (L - c3)) & tail) != 0;
                        const bool right_bad = strand ? low_bad : high_bad, left_bad = strand ? high_bad : low_bad;
                        if (!right_bad) {
                            atomicAdd(slot + 6, 1u);
                            ++wadds;
                        }
                        if (!left_bad) {
                            atomicAdd(slot + 7, 1u);
                            ++wadds;
                        }
                    }
                }
            }
        }
        if (op == 0) ++ni;
        else if (op == 1) ++nx;
        else ++ng;
        if (op != 0) --d;
        if (op != 3) --r;
        if (op != 2) --j;
    }
    if (run) atomicOr(a.fail, 1u);   // (a script does not begin with D)
    a.a_start[oi] = p.start + j;
    a.nident[oi] = ni;
    a.mismatch[oi] = nx;
    a.gaps[oi] = ng;
    if (piled) {
        atomicAdd(s.depth + (uint64_t)p.query * s.n_groups + lab, 1u);
        atomicAdd(tally + PS_ADDS, (unsigned long long)adds);
        atomicAdd(wtally + WS_WINDOWS, (unsigned long long)seen);
        atomicAdd(wtally + WS_ADDS, (unsigned long long)wadds);
    }
    atomicAdd(tally + (piled ? PS_PILED : labelled ? PS_FILTERED : PS_LEFT_OUT), 1ull);
}

// pairs [p0, p1) of the list, one lane each; the workgroup's counters go to the sinks' in one add each
__global__ __launch_bounds__(SQ_TPB) void k_al_walk_win(AlArgs a, PileSink s, WinSink ws, uint64_t p0, uint64_t p1)
{
    __shared__ unsigned long long tally[PS_N], wtally[WS_N];
    if (threadIdx.x < PS_N) tally[threadIdx.x] = 0;
    if (threadIdx.x < WS_N) wtally[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = p0 + (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x;
    if (i < p1) win_pair(a, s, ws, i, tally, wtally);
    __syncthreads();
    if (threadIdx.x < PS_N && tally[threadIdx.x]) atomicAdd(s.stat + threadIdx.x, tally[threadIdx.x]);
    if (threadIdx.x < WS_N && wtally[threadIdx.x]) atomicAdd(ws.stat + threadIdx.x, wtally[threadIdx.x]);
}

// One thread per (row, length, group) of the window table, after the last walk: MM0 = depth - (MM1 + .. + GAPPED) at every window
// start u <= m - L, and MM0 more to FWD_OK and REV_OK (a perfect window is both).  Rows behind m - L stay 0.
__global__ __launch_bounds__(SQ_TPB) void k_win_finish(uint32_t *__restrict__ table, const uint32_t *__restrict__ depth, const uint64_t *__restrict__ qoff, uint64_t nq,
                                                       uint32_t n_groups, WinSink ws, uint64_t x0, uint64_t x1, uint32_t *__restrict__ fail)
{
    const uint64_t x = x0 + (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x;
    if (x >= x1) return;
    const uint64_t per_row = (uint64_t)ws.n_lengths * n_groups, row = x / per_row;
    const uint32_t l = (uint32_t)((x % per_row) / n_groups), g = (uint32_t)(x % n_groups);
    // the query of the row: the last q with qoff[q] <= row (empty queries share an offset with the next one)
    uint64_t lo = 0, hi = nq;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (qoff[mid] <= row) lo = mid;
        else hi = mid;
    }
    const uint64_t m = qoff[lo + 1] - qoff[lo], u = row - qoff[lo];
    if (row < qoff[lo] || u >= m) {
        atomicOr(fail, 1u);
        return;
    }
    const uint32_t L = ws.len[l];
    if (m < L || u > m - L) return;
    uint32_t *const c = table + x * WIN_CLASSES;
    const uint32_t other = c[1] + c[2] + c[3] + c[4] + c[5], dep = depth[lo * n_groups + g];
    if (other > dep) {
        atomicOr(fail, 1u);
        return;
    }
    const uint32_t mm0 = dep - other;
    c[0] = mm0;
    c[6] += mm0;
    c[7] += mm0;
}

// script of pair x: ops [off[x], off[x + 1]) of the output, the last bytes of its padded slot
__global__ __launch_bounds__(SQ_TPB) void k_al_compact(uint64_t b0, uint64_t total, const uint64_t *__restrict__ off, uint32_t n, const uint64_t *__restrict__ pad_end,
                                                       const uint8_t *__restrict__ padded, uint8_t *__restrict__ out)
{
    const uint64_t x = b0 + (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x;
    if (x >= total) return;
    uint32_t lo = 0, hi = n;   // the last pair whose offset is <= x (empty scripts are stepped over)
    while (lo + 1 < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    out[x] = padded[pad_end[lo] - (off[lo + 1] - x)];
}

}  // namespace

void align_device(const Runs &runs, const QueryPack &P, const sw_infix_pair *d_pairs, const uint32_t *d_out_idx, uint64_t n, const uint32_t *d_dist,
                  const uint32_t *d_end, uint32_t *const out[4], uint8_t *d_ops, const uint64_t *d_ops_end, AlignStats &st, const PileSink *pile,
                  const WinSink *win)
{
    if (!n) return;
    if (win && !pile) raise(SW_ERR_RUNTIME, "internal error: the window walk needs the pileup's sink");
    if (n > SQ_MAX_LIST) raise(SW_ERR_VALUE, "infix alignments: %llu pairs exceed one launch of the list kernels (%llu)", (unsigned long long)n, (unsigned long long)SQ_MAX_LIST);
    const hipStream_t stream = HIT_STREAM;
    const uint32_t cap = ed_cap_blocks();
    // the scratch's budget changes speed only; SEQWIN_AMD_ALN_SCRATCH_KB (test library) sets it
    uint64_t budget = ALN_SCRATCH_BYTES;
    if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_ALN_SCRATCH_KB")) budget = env_u64(e, budget >> 10) << 10;
    const uint64_t budget_cells = std::max<uint64_t>(budget / ALN_CELL_BYTES, 1);

    // sizes on the device, their prefix sums and the rounds on the host
    DevArray<uint64_t> d_cells(n + 1);
    DevArray<uint8_t> d_cls(n);
    DevArray<unsigned long long> d_stat(1);
    SW_HIP(hipMemsetAsync(d_stat.p, 0, 8, stream));
    hipLaunchKernelGGL(k_al_size, dim3(sq_blocks(n)), dim3(SQ_TPB), 0, stream, d_pairs, d_out_idx, (const uint64_t *)P.off.p, d_dist, d_end, n, cap, d_cells.p, d_cls.p,
                       d_stat.p);
    SW_HIP(hipGetLastError());
    std::vector<uint64_t> off(n + 1);
    std::vector<uint8_t> cls(n);
    unsigned long long longest_striped = 0;
    SW_HIP(hipMemcpyAsync(off.data(), d_cells.p, n * 8, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipMemcpyAsync(cls.data(), d_cls.p, n, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipMemcpyAsync(&longest_striped, d_stat.p, 8, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    uint64_t sum = 0, largest = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t c = off[i];
        largest = std::max(largest, c);
        off[i] = sum;
        sum += c;
    }
    off[n] = sum;
    SW_HIP(hipMemcpyAsync(d_cells.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream));
    std::vector<uint64_t> bounds{0};   // round r: pairs [bounds[r], bounds[r + 1])
    uint64_t peak_cells = 0, own = 0;
    for (uint64_t p0 = 0; p0 < n;) {
        uint64_t p1 = p0;
        while (p1 < n && off[p1 + 1] - off[p0] <= budget_cells) ++p1;
        if (p1 == p0) {   // one pair above the budget: a scratch of its own size
            ++p1;
            ++own;
        }
        peak_cells = std::max(peak_cells, off[p1] - off[p0]);
        bounds.push_back(p1);
        p0 = p1;
    }
    DevArray<uint64_t> pv(peak_cells), mv(peak_cells);
    DevArray<uint32_t> sc(peak_cells);

    AlArgs a{};
    a.t = table_of(runs);
    for (int s = 0; s < 2; ++s) {
        a.codes[s] = P.codes[s].p;
        a.valid[s] = P.valid[s].p;
    }
    a.qoff = P.off.p;
    a.pairs = d_pairs;
    a.out_idx = d_out_idx;
    a.dist = d_dist;
    a.end = d_end;
    a.cell_off = d_cells.p;
    a.pv = pv.p;
    a.mv = mv.p;
    a.sc = sc.p;
    a.a_start = out[0];
    a.nident = out[1];
    a.mismatch = out[2];
    a.gaps = out[3];
    a.ops = d_ops;
    a.ops_end = d_ops_end;
    const uint64_t max_threads = (uint64_t)launch_blocks(SQ_BLOCKS_ENV) * SQ_TPB;
    uint32_t gs = 1;   // striped route: the largest power of two <= cap lanes per pair
    while (gs * 2 <= cap) gs *= 2;
    DevArray<uint8_t> carry;
    DevArray<uint32_t> d_list, d_fail(1);
    SW_HIP(hipMemsetAsync(d_fail.p, 0, 4, stream));
    a.fail = d_fail.p;
    Event e0, e1, e2;
    uint64_t striped = 0, launches = 0;
    for (size_t r = 0; r + 1 < bounds.size(); ++r) {
        const uint64_t p0 = bounds[r], p1 = bounds[r + 1];
        // the round's pairs by class, one list behind the other
        std::vector<uint32_t> list;
        uint64_t at[ED_CLASSES + 1] = {};
        for (uint64_t i = p0; i < p1; ++i)
            if (cls[i] != ALN_NO_CLASS) ++at[cls[i] + 1];
        for (uint32_t c = 0; c < ED_CLASSES; ++c) at[c + 1] += at[c];
        list.resize(at[ED_CLASSES]);
        {
            uint64_t fill[ED_CLASSES];
            memcpy(fill, at, sizeof fill);
            for (uint64_t i = p0; i < p1; ++i)
                if (cls[i] != ALN_NO_CLASS) list[fill[cls[i]]++] = (uint32_t)i;
        }
        d_list.alloc(list.size());
        if (!list.empty()) SW_HIP(hipMemcpyAsync(d_list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, stream));
        a.round_base = off[p0];
        SW_HIP(hipEventRecord(e0, stream));
        for (uint32_t c = 0; c + 1 < ED_CLASSES; ++c) {   // register route, g = 2^c lanes per pair
            const uint64_t cnt = at[c + 1] - at[c], g = 1ull << c, per_launch = std::max<uint64_t>(max_threads / g, 1);
            for (uint64_t x0 = 0; x0 < cnt; x0 += per_launch, ++launches) {
                a.list = d_list.p + at[c] + x0;
                a.count = std::min<uint64_t>(per_launch, cnt - x0);
                a.g = (uint32_t)g;
                hipLaunchKernelGGL(k_al_store, dim3(sq_blocks(a.count * g)), dim3(SQ_TPB), 0, stream, a);
                SW_HIP(hipGetLastError());
            }
        }
        if (const uint64_t cnt = at[ED_CLASSES] - at[ED_CLASSES - 1]) {
            const uint32_t groups = (uint32_t)std::min<uint64_t>({cnt, (uint64_t)ED_STRIPE_GROUPS, std::max<uint64_t>(max_threads / gs, 1)});
            a.carry_stride = ((uint64_t)longest_striped + 15) & ~7ull;
            if (carry.n < (uint64_t)groups * a.carry_stride) carry.alloc((uint64_t)groups * a.carry_stride);
            a.carry = carry.p;
            a.list = d_list.p + at[ED_CLASSES - 1];
            a.count = cnt;
            a.g = gs;
            hipLaunchKernelGGL(k_al_store_striped, dim3(sq_blocks((uint64_t)groups * gs)), dim3(SQ_TPB), 0, stream, a, groups);
            SW_HIP(hipGetLastError());
            ++launches;
            striped += cnt;
        }
        SW_HIP(hipEventRecord(e1, stream));
        for (uint64_t x0 = p0; x0 < p1; x0 += max_threads) {
            const uint64_t x1 = std::min<uint64_t>(p1, x0 + max_threads);
            if (win) hipLaunchKernelGGL(k_al_walk_win, dim3(sq_blocks(x1 - x0)), dim3(SQ_TPB), 0, stream, a, *pile, *win, x0, x1);
            else if (pile) hipLaunchKernelGGL(k_al_walk_pile, dim3(sq_blocks(x1 - x0)), dim3(SQ_TPB), 0, stream, a, *pile, x0, x1);
            else hipLaunchKernelGGL(k_al_walk, dim3(sq_blocks(x1 - x0)), dim3(SQ_TPB), 0, stream, a, x0, x1);
            SW_HIP(hipGetLastError());
        }
        SW_HIP(hipEventRecord(e2, stream));
        uint32_t failed = 0;
        SW_HIP(hipMemcpyAsync(&failed, d_fail.p, 4, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));   // (the list is the host's until here; the scratch is the next round's)
        if (failed) raise(SW_ERR_RUNTIME, "internal error: a traceback left the band its distance allows");
        float ms = 0;
        SW_HIP(hipEventElapsedTime(&ms, e0, e1));
        st.ms[0] += ms;
        SW_HIP(hipEventElapsedTime(&ms, e1, e2));
        st.ms[1] += ms;
    }
    st.counters[0] += n;
    st.counters[1] += bounds.size() - 1;
    st.counters[2] += striped;
    st.counters[3] += own;
    st.counters[4] = std::max(st.counters[4], peak_cells * ALN_CELL_BYTES);
    st.counters[6] = std::max(st.counters[6], largest * ALN_CELL_BYTES);
    st.counters[7] += launches;
}

// ---- the pileup's tables ---------------------------------------------------------------------------------
// n_piles: the pairs of the call or the assemblies of the batch -- the most one counter can be added to
void check_pile_args(const char *what, uint64_t n_groups, uint64_t max_dist_permille, const uint8_t *labels, uint64_t n_labels, uint64_t n_piles,
                     const uint64_t *offsets, uint64_t nq)
{
    if (n_groups < 1 || n_groups > 8) raise(SW_ERR_VALUE, "%s: the pileup takes 1..8 groups (got %llu)", what, (unsigned long long)n_groups);
    if (max_dist_permille > 1000) raise(SW_ERR_VALUE, "%s: max_dist_permille must lie in 0..1000 (got %llu)", what, (unsigned long long)max_dist_permille);
    if (n_labels && !labels) raise(SW_ERR_VALUE, "%s: a NULL handle or array", what);
    for (uint64_t i = 0; i < n_labels; ++i)
        if (labels[i] >= n_groups && labels[i] != PILE_LEAVE_OUT)
            raise(SW_ERR_VALUE, "%s: group label %u at %llu is neither below the %llu groups nor 255 (leave out)", what, (unsigned)labels[i], (unsigned long long)i,
                  (unsigned long long)n_groups);
    uint64_t max_q = 0;
    for (uint64_t q = 0; q < nq; ++q) max_q = std::max(max_q, offsets[q + 1] - offsets[q]);
    if (n_piles && max_q && (n_piles >= (1ull << 32) || max_q >= (1ull << 32) || n_piles * max_q >= (1ull << 32)))
        raise(SW_ERR_VALUE, "%s: %llu pairs or assemblies times the longest query (%llu) do not fit the pileup's 32-bit counters", what,
              (unsigned long long)n_piles, (unsigned long long)max_q);
}

void pile_begin(sw_pileup &p, int device, const uint64_t *offsets, uint64_t nq, uint64_t n_groups, uint64_t max_dist_permille, const uint8_t *labels,
                uint64_t n_labels, uint64_t group_mod)
{
    const hipStream_t stream = HIT_STREAM;
    p.device = device;
    p.nq = nq;
    p.n_groups = n_groups;
    p.off.assign(offsets, offsets + nq + 1);
    const uint64_t cells = p.off[nq] * n_groups * PILE_CLASSES;
    p.table.alloc(cells);
    p.depth.alloc(nq * n_groups);
    p.labels.alloc(n_labels);
    p.stat.alloc(PS_N);
    if (cells) SW_HIP(hipMemsetAsync(p.table.p, 0, cells * 4, stream));
    if (nq) SW_HIP(hipMemsetAsync(p.depth.p, 0, nq * n_groups * 4, stream));
    SW_HIP(hipMemsetAsync(p.stat.p, 0, PS_N * sizeof(unsigned long long), stream));
    if (n_labels) SW_HIP(hipMemcpyAsync(p.labels.p, labels, n_labels, hipMemcpyHostToDevice, stream));
    SW_HIP(hipStreamSynchronize(stream));   // (the labels are the caller's)
    p.sink = PileSink{p.table.p, p.depth.p, p.labels.p, group_mod, (uint32_t)n_groups, (uint32_t)max_dist_permille, p.stat.p};
    p.counters[4] = cells * 4;
}

void pile_finish(sw_pileup &p, double walk_ms)
{
    unsigned long long st[PS_N] = {};
    SW_HIP(hipMemcpyAsync(st, p.stat.p, sizeof st, hipMemcpyDeviceToHost, HIT_STREAM));
    SW_HIP(hipStreamSynchronize(HIT_STREAM));
    for (int x = 0; x < PS_N; ++x) p.counters[x] = st[x];
    p.ms = walk_ms;
    p.labels.release();
    p.stat.release();
    p.sink = PileSink{};
}

// ---- the oligo windows' table -----------------------------------------------------------------------------
void check_win_args(const char *what, const uint32_t *lengths, uint64_t n_lengths, uint64_t max_mismatch, uint64_t three_prime)
{
    if (n_lengths < 1 || n_lengths > WIN_MAX_LENGTHS)
        raise(SW_ERR_VALUE, "%s: the windows take 1..%u lengths (got %llu)", what, WIN_MAX_LENGTHS, (unsigned long long)n_lengths);
    if (!lengths) raise(SW_ERR_VALUE, "%s: a NULL handle or array", what);
    uint32_t shortest = 32;
    for (uint64_t i = 0; i < n_lengths; ++i) {
        if (lengths[i] < 8 || lengths[i] > 32) raise(SW_ERR_VALUE, "%s: window length %u lies outside 8..32", what, lengths[i]);
        for (uint64_t j = 0; j < i; ++j)
            if (lengths[j] == lengths[i]) raise(SW_ERR_VALUE, "%s: window length %u is given twice", what, lengths[i]);
        shortest = std::min(shortest, lengths[i]);
    }
    if (max_mismatch > 8 || max_mismatch >= shortest)
        raise(SW_ERR_VALUE, "%s: max_mismatch must lie in 0..8 and below the shortest window length %u (got %llu)", what, shortest,
              (unsigned long long)max_mismatch);
    if (three_prime > 8) raise(SW_ERR_VALUE, "%s: three_prime must lie in 0..8 (got %llu)", what, (unsigned long long)three_prime);
}

void win_begin(sw_windows &w, int device, const uint64_t *offsets, uint64_t nq, uint64_t n_groups, const uint32_t *lengths, uint64_t n_lengths,
               uint64_t max_mismatch, uint64_t three_prime)
{
    const hipStream_t stream = HIT_STREAM;
    w.device = device;
    w.nq = nq;
    w.n_groups = n_groups;
    w.n_lengths = n_lengths;
    w.max_mismatch = max_mismatch;
    w.three_prime = three_prime;
    w.off.assign(offsets, offsets + nq + 1);
    const uint64_t cells = w.off[nq] * n_lengths * n_groups * WIN_CLASSES;   // (below 2^32 rows * 8 * 8 * 8: no overflow in 64 bits)
    w.table.alloc(cells);
    w.d_off.alloc(nq + 1);
    w.stat.alloc(WS_N);
    if (cells) SW_HIP(hipMemsetAsync(w.table.p, 0, cells * 4, stream));
    SW_HIP(hipMemcpyAsync(w.d_off.p, w.off.data(), (nq + 1) * 8, hipMemcpyHostToDevice, stream));
    SW_HIP(hipMemsetAsync(w.stat.p, 0, WS_N * sizeof(unsigned long long), stream));
    SW_HIP(hipStreamSynchronize(stream));
    w.sink = WinSink{};
    w.sink.table = w.table.p;
    for (uint64_t i = 0; i < n_lengths; ++i) w.sink.len[i] = w.lengths[i] = lengths[i];
    w.sink.n_lengths = (uint32_t)n_lengths;
    w.sink.max_mismatch = (uint32_t)max_mismatch;
    w.sink.three_prime = (uint32_t)three_prime;
    w.sink.stat = w.stat.p;
    w.counters[2] = cells * 4;
}

void win_finish(sw_windows &w, const sw_pileup &p, double walk_ms)
{
    const hipStream_t stream = HIT_STREAM;
    const uint64_t items = w.off[w.nq] * w.n_lengths * w.n_groups;
    DevArray<uint32_t> d_fail(1);
    SW_HIP(hipMemsetAsync(d_fail.p, 0, 4, stream));
    Event e0, e1;
    SW_HIP(hipEventRecord(e0, stream));
    const uint64_t max_threads = (uint64_t)launch_blocks(SQ_BLOCKS_ENV) * SQ_TPB;
    for (uint64_t x0 = 0; x0 < items; x0 += max_threads) {
        const uint64_t x1 = std::min<uint64_t>(items, x0 + max_threads);
        hipLaunchKernelGGL(k_win_finish, dim3(sq_blocks(x1 - x0)), dim3(SQ_TPB), 0, stream, w.table.p, (const uint32_t *)p.depth.p, (const uint64_t *)w.d_off.p, w.nq,
                           (uint32_t)w.n_groups, w.sink, x0, x1, d_fail.p);
        SW_HIP(hipGetLastError());
    }
    SW_HIP(hipEventRecord(e1, stream));
    unsigned long long st[WS_N] = {};
    uint32_t failed = 0;
    SW_HIP(hipMemcpyAsync(st, w.stat.p, sizeof st, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipMemcpyAsync(&failed, d_fail.p, 4, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    if (failed) raise(SW_ERR_RUNTIME, "internal error: a window's classes exceed the depth of its query");
    float ms = 0;
    SW_HIP(hipEventElapsedTime(&ms, e0, e1));
    w.counters[WS_WINDOWS] = st[WS_WINDOWS];
    w.counters[WS_ADDS] = st[WS_ADDS];
    w.ms[0] = walk_ms;
    w.ms[1] = ms;
    w.d_off.release();
    w.stat.release();
    w.sink = WinSink{};
}

}  // namespace sw

struct sw_ops {
    int device = 0;
    uint64_t n = 0, bytes = 0;
    sw::DevArray<uint64_t> off;   // [n + 1]
    sw::DevArray<uint8_t> ops;
};

using namespace sw;

extern "C" {

int sw_batch_infix_alignments(const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs, uint64_t n,
                              uint32_t *dist, uint32_t *end, uint32_t *a_start, uint32_t *nident, uint32_t *mismatch, uint32_t *gaps, sw_ops **ops,
                              uint64_t *counters, double *ms)
{
    return guarded([&] {
        check_infix_pairs("infix alignments", b, offsets, blob, n_queries, pairs, n, dist && end && a_start && nident && mismatch && gaps);
        StreamScope scope(HIT_STREAM);
        DevRuns runs(*b);
        const uint64_t total = n_queries ? offsets[n_queries] : 0;
        DevArray<uint8_t> text(total);
        if (total) SW_HIP(hipMemcpyAsync(text.p, blob, total, hipMemcpyHostToDevice, HIT_STREAM));
        QueryPack P;
        pack_queries(text.p, offsets, n_queries, P);
        DevArray<sw_infix_pair> d_pairs(n);
        DevArray<uint32_t> d_dist(n), d_end(n), d_out[4];
        for (auto &o : d_out) o.alloc(n);
        if (n) SW_HIP(hipMemcpyAsync(d_pairs.p, pairs, n * sizeof(sw_infix_pair), hipMemcpyHostToDevice, HIT_STREAM));
        double dms[1] = {};
        infix_device(runs_of(runs.t), P, d_pairs.p, nullptr, n, d_dist.p, d_end.p, nullptr, dms);
        if (n) {
            SW_HIP(hipMemcpy(dist, d_dist.p, n * 4, hipMemcpyDeviceToHost));
            SW_HIP(hipMemcpy(end, d_end.p, n * 4, hipMemcpyDeviceToHost));
        }
        // scripts: padded slots of |query| + dist bytes, filled from their ends
        std::vector<uint64_t> pad_end(n);
        DevArray<uint8_t> padded;
        DevArray<uint64_t> d_pad_end;
        if (ops) {
            uint64_t sum = 0;
            for (uint64_t i = 0; i < n; ++i) pad_end[i] = sum += offsets[pairs[i].query + 1] - offsets[pairs[i].query] + dist[i];
            padded.alloc(sum);
            d_pad_end.alloc(n);
            if (n) SW_HIP(hipMemcpyAsync(d_pad_end.p, pad_end.data(), n * 8, hipMemcpyHostToDevice, HIT_STREAM));
        }
        AlignStats st;
        uint32_t *const out[4] = {d_out[0].p, d_out[1].p, d_out[2].p, d_out[3].p};
        align_device(runs_of(runs.t), P, d_pairs.p, nullptr, n, d_dist.p, d_end.p, out, ops ? padded.p : nullptr, d_pad_end.p, st);
        uint32_t *const host[4] = {a_start, nident, mismatch, gaps};
        if (n)
            for (int f = 0; f < 4; ++f) SW_HIP(hipMemcpy(host[f], d_out[f].p, n * 4, hipMemcpyDeviceToHost));
        if (ops) {
            std::unique_ptr<sw_ops> o(new sw_ops);
            o->device = b->device;
            o->n = n;
            std::vector<uint64_t> off(n + 1, 0);   // the script of pair i: |query| + #D entries, #D = (end - a_start) - (nident + mismatch)
            for (uint64_t i = 0; i < n; ++i)
                off[i + 1] = off[i] + (offsets[pairs[i].query + 1] - offsets[pairs[i].query]) + ((uint64_t)(end[i] - a_start[i]) - nident[i] - mismatch[i]);
            o->bytes = off[n];
            o->off.alloc(n + 1);
            o->ops.alloc(o->bytes);
            SW_HIP(hipMemcpyAsync(o->off.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, HIT_STREAM));
            const uint64_t per = (uint64_t)launch_blocks(SQ_BLOCKS_ENV) * SQ_TPB;
            for (uint64_t b0 = 0; b0 < o->bytes; b0 += per) {
                const uint64_t cnt = std::min<uint64_t>(per, o->bytes - b0);
                hipLaunchKernelGGL(k_al_compact, dim3(sq_blocks(cnt)), dim3(SQ_TPB), 0, HIT_STREAM, b0, b0 + cnt, (const uint64_t *)o->off.p, (uint32_t)n,
                                   (const uint64_t *)d_pad_end.p, (const uint8_t *)padded.p, o->ops.p);
                SW_HIP(hipGetLastError());
            }
            SW_HIP(hipStreamSynchronize(HIT_STREAM));
            st.counters[5] = o->bytes;
            *ops = o.release();
        }
        if (counters) memcpy(counters, st.counters, sizeof st.counters);
        if (ms) {
            ms[0] = dms[0];
            ms[1] = st.ms[0];
            ms[2] = st.ms[1];
        }
    });
}

int sw_ops_sizes(const sw_ops *o, uint64_t *n, uint64_t *bytes)
{
    return guarded([&] {
        if (!o) raise(SW_ERR_VALUE, "infix alignments: a NULL handle");
        if (n) *n = o->n;
        if (bytes) *bytes = o->bytes;
    });
}

int sw_ops_export(const sw_ops *o, uint64_t *offsets, uint8_t *ops)
{
    return guarded([&] {
        if (!o) raise(SW_ERR_VALUE, "infix alignments: a NULL handle");
        require_device(o->device, "the scripts");
        if (offsets) SW_HIP(hipMemcpy(offsets, o->off.p, (o->n + 1) * 8, hipMemcpyDeviceToHost));
        if (ops && o->bytes) SW_HIP(hipMemcpy(ops, o->ops.p, o->bytes, hipMemcpyDeviceToHost));
    });
}

void sw_ops_free(sw_ops *o)
{
    delete o;
}

// the window arguments of a call; without them the call is the pileup's
struct WinSpec {
    const uint32_t *lengths;
    uint64_t n_lengths, max_mismatch, three_prime;
    sw_windows **out;
};

static int infix_pileup_entry(const char *what, const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs, uint64_t n,
                              const uint8_t *pair_group, uint64_t n_groups, uint64_t max_dist_permille, uint32_t *dist, uint32_t *end, uint32_t *a_start,
                              uint32_t *nident, uint32_t *mismatch, uint32_t *gaps, sw_pileup **out, uint64_t *counters, double *ms, const WinSpec *win)
{
    return guarded([&] {
        check_queries(what, offsets, blob, n_queries);
        check_pile_args(what, n_groups, max_dist_permille, pair_group, n, n, offsets, n_queries);
        if (win) check_win_args(what, win->lengths, win->n_lengths, win->max_mismatch, win->three_prime);
        if (!out || (win && !win->out)) raise(SW_ERR_VALUE, "%s: a NULL handle or array", what);
        check_infix_pairs(what, b, offsets, blob, n_queries, pairs, n, dist && end && a_start && nident && mismatch && gaps);
        StreamScope scope(HIT_STREAM);
        DevRuns runs(*b);
        const uint64_t total = n_queries ? offsets[n_queries] : 0;
        DevArray<uint8_t> text(total);
        if (total) SW_HIP(hipMemcpyAsync(text.p, blob, total, hipMemcpyHostToDevice, HIT_STREAM));
        QueryPack P;
        pack_queries(text.p, offsets, n_queries, P);
        DevArray<sw_infix_pair> d_pairs(n);
        DevArray<uint32_t> d_dist(n), d_end(n), d_out[4];
        for (auto &o : d_out) o.alloc(n);
        if (n) SW_HIP(hipMemcpyAsync(d_pairs.p, pairs, n * sizeof(sw_infix_pair), hipMemcpyHostToDevice, HIT_STREAM));
        double dms[1] = {};
        infix_device(runs_of(runs.t), P, d_pairs.p, nullptr, n, d_dist.p, d_end.p, nullptr, dms);
        const uint64_t no_query[1] = {0};
        std::unique_ptr<sw_pileup> p(new sw_pileup);
        pile_begin(*p, b->device, n_queries ? offsets : no_query, n_queries, n_groups, max_dist_permille, pair_group, n, 0);
        std::unique_ptr<sw_windows> w(win ? new sw_windows : nullptr);
        if (win) win_begin(*w, b->device, n_queries ? offsets : no_query, n_queries, n_groups, win->lengths, win->n_lengths, win->max_mismatch, win->three_prime);
        AlignStats st;
        uint32_t *const dev[4] = {d_out[0].p, d_out[1].p, d_out[2].p, d_out[3].p};
        align_device(runs_of(runs.t), P, d_pairs.p, nullptr, n, d_dist.p, d_end.p, dev, nullptr, nullptr, st, &p->sink, win ? &w->sink : nullptr);
        if (win) win_finish(*w, *p, st.ms[1]);
        pile_finish(*p, st.ms[1]);
        uint32_t *const host[6] = {dist, end, a_start, nident, mismatch, gaps};
        const uint32_t *const from[6] = {d_dist.p, d_end.p, d_out[0].p, d_out[1].p, d_out[2].p, d_out[3].p};
        if (n)
            for (int f = 0; f < 6; ++f) SW_HIP(hipMemcpy(host[f], from[f], n * 4, hipMemcpyDeviceToHost));
        if (counters) memcpy(counters, st.counters, sizeof st.counters);
        if (ms) {
            ms[0] = dms[0];
            ms[1] = st.ms[0];
            ms[2] = st.ms[1];
        }
        *out = p.release();
        if (win) *win->out = w.release();
    });
}

int sw_batch_infix_pileup(const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs, uint64_t n,
                          const uint8_t *pair_group, uint64_t n_groups, uint64_t max_dist_permille, uint32_t *dist, uint32_t *end, uint32_t *a_start,
                          uint32_t *nident, uint32_t *mismatch, uint32_t *gaps, sw_pileup **out, uint64_t *counters, double *ms)
{
    return infix_pileup_entry("infix pileup", b, offsets, blob, n_queries, pairs, n, pair_group, n_groups, max_dist_permille, dist, end, a_start, nident, mismatch,
                              gaps, out, counters, ms, nullptr);
}

int sw_batch_infix_windows(const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs, uint64_t n,
                           const uint8_t *pair_group, uint64_t n_groups, uint64_t max_dist_permille, const uint32_t *lengths, uint64_t n_lengths,
                           uint64_t max_mismatch, uint64_t three_prime, uint32_t *dist, uint32_t *end, uint32_t *a_start, uint32_t *nident,
                           uint32_t *mismatch, uint32_t *gaps, sw_pileup **out, sw_windows **windows, uint64_t *counters, double *ms)
{
    const WinSpec win{lengths, n_lengths, max_mismatch, three_prime, windows};
    return infix_pileup_entry("infix windows", b, offsets, blob, n_queries, pairs, n, pair_group, n_groups, max_dist_permille, dist, end, a_start, nident, mismatch,
                              gaps, out, counters, ms, &win);
}

static const sw_windows &windows_of(const sw_windows *w)
{
    if (!w) raise(SW_ERR_VALUE, "windows: a NULL handle");
    return *w;
}

int sw_windows_sizes(const sw_windows *w, uint64_t *n_queries, uint64_t *total_bases, uint64_t *n_groups, uint64_t *n_lengths, uint64_t *max_mismatch,
                     uint64_t *three_prime)
{
    return guarded([&] {
        const sw_windows &x = windows_of(w);
        if (n_queries) *n_queries = x.nq;
        if (total_bases) *total_bases = x.off[x.nq];
        if (n_groups) *n_groups = x.n_groups;
        if (n_lengths) *n_lengths = x.n_lengths;
        if (max_mismatch) *max_mismatch = x.max_mismatch;
        if (three_prime) *three_prime = x.three_prime;
    });
}

int sw_windows_lengths(const sw_windows *w, uint32_t *lengths)
{
    return guarded([&] {
        const sw_windows &x = windows_of(w);
        if (!lengths) raise(SW_ERR_VALUE, "windows: a NULL handle or array");
        for (uint64_t i = 0; i < x.n_lengths; ++i) lengths[i] = x.lengths[i];
    });
}

int sw_windows_export(const sw_windows *w, uint64_t q0, uint64_t q1, uint32_t *out)
{
    return guarded([&] {
        const sw_windows &x = windows_of(w);
        if (q0 > q1 || q1 > x.nq)
            raise(SW_ERR_VALUE, "windows: queries [%llu, %llu) lie outside the %llu queries", (unsigned long long)q0, (unsigned long long)q1, (unsigned long long)x.nq);
        const uint64_t per = x.n_lengths * x.n_groups * WIN_CLASSES, cells = (x.off[q1] - x.off[q0]) * per;
        if (!cells) return;
        if (!out) raise(SW_ERR_VALUE, "windows: a NULL handle or array");
        require_device(x.device, "the windows");
        SW_HIP(hipMemcpy(out, x.table.p + x.off[q0] * per, cells * 4, hipMemcpyDeviceToHost));
    });
}

int sw_windows_stats(const sw_windows *w, uint64_t *counters, double *ms)
{
    return guarded([&] {
        const sw_windows &x = windows_of(w);
        if (counters) memcpy(counters, x.counters, sizeof x.counters);
        if (ms) memcpy(ms, x.ms, sizeof x.ms);
    });
}

void sw_windows_free(sw_windows *w)
{
    delete w;
}

static const sw_pileup &pile_of(const sw_pileup *p)
{
    if (!p) raise(SW_ERR_VALUE, "pileup: a NULL handle");
    return *p;
}

int sw_pileup_sizes(const sw_pileup *p, uint64_t *n_queries, uint64_t *total_bases, uint64_t *n_groups)
{
    return guarded([&] {
        const sw_pileup &x = pile_of(p);
        if (n_queries) *n_queries = x.nq;
        if (total_bases) *total_bases = x.off[x.nq];
        if (n_groups) *n_groups = x.n_groups;
    });
}

int sw_pileup_export(const sw_pileup *p, uint64_t q0, uint64_t q1, uint32_t *out)
{
    return guarded([&] {
        const sw_pileup &x = pile_of(p);
        if (q0 > q1 || q1 > x.nq)
            raise(SW_ERR_VALUE, "pileup: queries [%llu, %llu) lie outside the %llu queries", (unsigned long long)q0, (unsigned long long)q1, (unsigned long long)x.nq);
        const uint64_t per = x.n_groups * PILE_CLASSES, cells = (x.off[q1] - x.off[q0]) * per;
        if (!cells) return;
        if (!out) raise(SW_ERR_VALUE, "pileup: a NULL handle or array");
        require_device(x.device, "the pileup");
        SW_HIP(hipMemcpy(out, x.table.p + x.off[q0] * per, cells * 4, hipMemcpyDeviceToHost));
    });
}

int sw_pileup_depth(const sw_pileup *p, uint32_t *depth)
{
    return guarded([&] {
        const sw_pileup &x = pile_of(p);
        if (!x.nq) return;
        if (!depth) raise(SW_ERR_VALUE, "pileup: a NULL handle or array");
        require_device(x.device, "the pileup");
        SW_HIP(hipMemcpy(depth, x.depth.p, x.nq * x.n_groups * 4, hipMemcpyDeviceToHost));
    });
}

int sw_pileup_stats(const sw_pileup *p, uint64_t *counters, double *ms)
{
    return guarded([&] {
        const sw_pileup &x = pile_of(p);
        if (counters) memcpy(counters, x.counters, sizeof x.counters);
        if (ms) ms[0] = x.ms;
    });
}

void sw_pileup_free(sw_pileup *p)
{
    delete p;
}

int sw_hits_align_block(const sw_hits *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "best hits: a NULL handle");
        if (!h->aligned) raise(SW_ERR_VALUE, "best hits: these hits were made without the alignment (sw_batch_best_hits_aligned makes it)");
        if (field > 3) raise(SW_ERR_VALUE, "best hits: field %llu is none of a_start, nident, mismatch, gaps (0..3)", (unsigned long long)field);
        export_cells("best hits", "queries", h->device, "the hits", h->afield[field].p, h->nq, h->n_asm, r0, r1, c0, c1, out);
    });
}

int sw_hits_align_stats(const sw_hits *h, uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "best hits: a NULL handle");
        if (!h->aligned) raise(SW_ERR_VALUE, "best hits: these hits were made without the alignment (sw_batch_best_hits_aligned makes it)");
        if (counters) memcpy(counters, h->align.counters, sizeof h->align.counters);
        if (ms) memcpy(ms, h->align.ms, sizeof h->align.ms);
    });
}

}  // extern "C"
