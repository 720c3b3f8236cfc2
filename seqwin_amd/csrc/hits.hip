// hits.hip -- the best hit of every query in every assembly of a resident batch: seed vote + infix edit distance.
//
// Stands where markers.eval_markers (src/seqwin/markers.py:607-696) BLASTs every representative against every assembly and keeps the
// best hit's nident / mismatch / gaps of every (query, assembly) pair.  It has no counterpart in the reference, it is NOT BLAST and
// it fills none of MarkerMetrics (DESIGN.md section 3.2e is the specification; tests/tools/hits_host.py restates it).
//
// Layer A, infix edit distance (sw_batch_infix_distances): the pattern is a query (or its reverse complement), the text an interval
// of the batch; dist = min over the text's prefixes' ends of D[m][j] with a free start in the text, end = the first j of the minimum.
//   k_ix_pack      the query text as 2-bit codes and a validity plane, both strands, once per call
//   k_ix_classify  pairs with an empty side answered; the others listed by the power of two >= the query's blocks of 64 rows
//   k_ix           ed_pair's recurrence (seqs.hip) with three differences: the pattern is always the query, the top row's horizontal
//                  delta is 0, and the lane of the last block keeps the running minimum of the score and the first column that
//                  attains it; one strand.  k_ix_striped: queries above the block bound, with the HBM carry row
// Layer B, seed vote (sw_batch_best_hits): the query side is the screen's (screen_core.hpp); a canonical word that exactly one
// valid window of all query text has, and that is not its own reverse complement, is a seed.
//   k_hit_mult / k_hit_seeds   windows per distinct word; (query, offset, window-is-canonical) per seed
//   k_hit_probe    the batch's run / tile / lane walk (kmer_walk.hpp) with k_scr_probe's 16 grouped first-slot loads; a hit appends
//                  the 64-bit key (query | record | orientation | band) to the hit buffer: one atomic on the cursor per wave
//   per chunk of assemblies: the keys sorted over their used bits, run heads and lengths, k_hit_vote (score = run + next band's run,
//   the winner of a (query, assembly) by atomicMax of (score, ~run index): the smallest key wins a tie), k_hit_finish (the winner's
//   fields, its window as a pair of Layer A), and Layer A on the chunk's pairs.  A chunk whose hits overflow the buffer is redone in
//   two halves; one assembly that overflows it has the buffer doubled.
// Loci mode (sw_batch_best_hits_loci; tests/tools/loci_host.py restates it): behind a chunk's winners, every
//   run that is a local maximum of the score over two bands to either side (k_hit_peaks) is listed (k_hit_loci), measured and traced
//   like a winner; after the last chunk the lists are gathered into (query, record, orientation, band) order (k_loci_bounds, a scan,
//   k_loci_gather), duplicates are marked (k_hit_dups) and every cell is reduced by one thread (k_loci_reduce).
// Shared seeds (sw_batch_best_hits_shared; tests/tools/shared_seeds_host.py restates it): a word that up to
//   `seed_copies` windows of the query text have is a seed owned by each of them.  k_hit_keep (what the cap keeps, and the counts
//   of sw_hits_seed_stats), a scan, k_own_keys + a sort + k_own_fill (owner lists as CSR over the distinct words, placed by rank in
//   the sorted windows: no atomic decides a place), k_hit_probe_shared (a key per owner of a window's word: owners summed, one
//   append per wave, then the lists walked).  Everything behind the probe is the code above.
#include "hits_core.hpp"

namespace sw {
namespace {

constexpr uint32_t HIT_BAND_SHIFT = 6;                 // W = 64: part of the specification
constexpr uint64_t HIT_BUFFER_BYTES = 1ull << 30;      // hit keys and the sort's second buffer together: speed only, no measurement behind it
constexpr uint64_t HIT_MAX_KEYS = 1ull << 31;          // a run index and a score are 32-bit values
constexpr uint32_t IX_CLASSES = 8;                     // group widths 1, 2, ... 64, then the striped route
constexpr uint32_t IX_STRIPE_GROUPS = 1024;

uint32_t bits_of(uint64_t x)   // bits that hold 0 .. x
{
    uint32_t b = 0;
    while (b < 64 && (x >> b)) ++b;
    return b;
}

// ---- Layer A: the packed queries ------------------------------------------------------------------------------------------------
// Strand s of the query text: base x of query q lies at index off[q] + x of stream s; stream 1 holds the reverse complements.
// codes: 16 bases per word as the batch packs them; valid: a bit per base.
__global__ __launch_bounds__(SCR_TPB) void k_ix_pack(uint64_t base, uint64_t end, const uint8_t *__restrict__ text, const uint64_t *__restrict__ off, uint32_t nq,
                                                     uint64_t total, uint64_t groups, uint32_t *__restrict__ codes0, uint32_t *__restrict__ valid0,
                                                     uint32_t *__restrict__ codes1, uint32_t *__restrict__ valid1)
{
    const uint64_t w = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;   // (strand, group of 32 bases)
    if (w >= end) return;
    const bool rc = w >= groups;
    const uint64_t grp = rc ? w - groups : w;
    uint64_t g = grp * 32, c = 0;
    uint32_t v = 0, q = query_of(off, nq, g);
    for (uint32_t b = 0; b < 32 && g < total; ++b, ++g) {
        while (g >= off[q + 1]) ++q;   // (g < off[nq]: empty queries are stepped over)
        const uint64_t src = rc ? off[q + 1] - 1 - (g - off[q]) : g;
        const uint64_t code = base_code(text[src]);
        if (code < 4) {
            c |= (rc ? 3 - code : code) << (2 * b);
            v |= 1u << b;
        }
    }
    uint32_t *codes = rc ? codes1 : codes0, *valid = rc ? valid1 : valid0;
    codes[2 * grp] = (uint32_t)c;
    codes[2 * grp + 1] = (uint32_t)(c >> 32);
    valid[grp] = v;
}

}  // namespace

void pack_queries(const uint8_t *d_text, const uint64_t *offsets, uint64_t nq, QueryPack &P)
{
    const uint64_t total = nq ? offsets[nq] : 0, groups = (total + 31) / 32;
    P.nq = nq;
    P.off.alloc(nq + 1);
    if (nq) SW_HIP(hipMemcpyAsync(P.off.p, offsets, (nq + 1) * 8, hipMemcpyHostToDevice, HIT_STREAM));
    for (int s = 0; s < 2; ++s) {
        P.codes[s].alloc(2 * groups + 2);
        P.valid[s].alloc(groups + 1);
        SW_HIP(hipMemsetAsync(P.codes[s].p, 0, (2 * groups + 2) * 4, HIT_STREAM));
        SW_HIP(hipMemsetAsync(P.valid[s].p, 0, (groups + 1) * 4, HIT_STREAM));
    }
    if (groups)
        launch_1d(k_ix_pack, 2 * groups, HIT_STREAM, d_text, (const uint64_t *)P.off.p, (uint32_t)nq, total, groups, P.codes[0].p, P.valid[0].p, P.codes[1].p,
                  P.valid[1].p);
}

namespace {

// ---- Layer A: the kernels -------------------------------------------------------------------------------------------------------
struct IxArgs {
    RunTable t;
    const uint32_t *codes[2], *valid[2];
    const uint64_t *qoff;
    const sw_infix_pair *pairs;
    const uint32_t *out_idx;   // where pair i's results go (nullptr: i)
    const uint32_t *list;      // pair indices of this launch's class
    uint64_t count;
    uint32_t g;                // lanes per pair (a power of two <= 64)
    uint8_t *carry;            // striped route: one row of carry_stride bytes per group of the launch
    uint64_t carry_stride;     // a multiple of 8, >= the longest text + 8
    uint32_t *dist, *end;
};

// The group's lanes call this together.  Pattern: strand p.strand of query p.query, m >= 1 bases; text: [p.start, p.stop), n >= 1.
__device__ void infix_pair(const IxArgs &a, const sw_infix_pair &p, uint32_t g, uint32_t b, uint8_t *carry, uint32_t *dist_out, uint32_t *end_out)
{
    const RunTable &t = a.t;
    const uint64_t qbase = a.qoff[p.query];
    const uint32_t m = (uint32_t)(a.qoff[p.query + 1] - qbase), n = p.stop - p.start;
    const uint32_t *codes = a.codes[p.strand & 1u], *valid = a.valid[p.strand & 1u];
    const uint32_t nb = (m + 63) >> 6, n_stripes = (nb + g - 1) / g;
    const uint64_t tbase = t.rec_base[p.record] + p.start;
    uint32_t score = m, best = m, best_col = 0;   // column 0 of the table: no text consumed, D[m][0] = m
    RunMemo tm;
    for (uint32_t s = 0; s < n_stripes; ++s) {
        const uint32_t B = s * g + b, sb = nb - s * g < g ? nb - s * g : g;
        const bool active = b < sb, last_block = B == nb - 1, first = s == 0;
        const bool leaves_carry = active && b == sb - 1 && !last_block;
        uint64_t lo = 0, hi = 0, vm = 0;   // the block's rows as bit planes: low and high bit of the code, validity
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
        uint64_t Pv = ~0ull, Mv = 0;
        uint64_t tf = 0, cbuf = 0;   // lane 0: 32 columns of the text, 8 columns of the carry row
        uint32_t vf = 0;
        uint32_t msg = 0;            // column base [0,3) and delta [3,5)
        const uint32_t steps = n + sb - 1;
        for (uint32_t step = 0; step < steps; ++step) {
            uint32_t in = __shfl_up(msg, 1, g);
            if (b == 0 && step < n) {
                const uint32_t i = step & 31u;
                if (i == 0) {
                    const uint32_t cnt = n - step < 32 ? n - step : 32;
                    tf = load_codes(t.packed, tbase + step, cnt);
                    vf = valid32(t, p.record, p.start + step, cnt, tm);
                }
                const uint32_t cf = ((vf >> i) & 1u) ? (uint32_t)(tf >> (2 * i)) & 3u : 4u;
                uint32_t hf = 0;   // the top row of the table is 0 in every column: the match may start anywhere in the text
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
                if (last_block) {
                    score += of == 1 ? 1u : of == 2 ? 0xFFFFFFFFu : 0u;
                    if (score < best) {   // (strictly: the first column that attains the minimum stays)
                        best = score;
                        best_col = col + 1;
                    }
                } else if (leaves_carry) {
                    carry[col] = (uint8_t)of;   // (read by lane 0 of the next stripe, which is past this column there)
                }
                msg = cf | (of << 3);
            }
        }
        if (n_stripes > 1) __threadfence();   // the row is complete and visible before the next stripe reads it
        if (active && last_block) {
            *dist_out = best;
            *end_out = p.start + best_col;
        }
    }
}

// register route: group x of the launch does pair list[x]
__global__ __launch_bounds__(SQ_TPB) void k_ix(IxArgs a)
{
    const uint64_t tid = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x, grp = tid / a.g;
    if (grp >= a.count) return;   // (whole groups)
    const uint32_t i = a.list[grp], oi = a.out_idx ? a.out_idx[i] : i;
    infix_pair(a, a.pairs[i], a.g, (uint32_t)(tid % a.g), nullptr, a.dist + oi, a.end + oi);
}

// striped route: group x of the launch does pairs list[x], list[x + groups], ... with row x of the scratch
__global__ __launch_bounds__(SQ_TPB) void k_ix_striped(IxArgs a, uint32_t groups)
{
    const uint64_t tid = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x, grp = tid / a.g;
    if (grp >= groups) return;
    for (uint64_t x = grp; x < a.count; x += groups) {
        const uint32_t i = a.list[x], oi = a.out_idx ? a.out_idx[i] : i;
        infix_pair(a, a.pairs[i], a.g, (uint32_t)(tid % a.g), a.carry + grp * a.carry_stride, a.dist + oi, a.end + oi);
        __threadfence();   // (the row is reused by the group's next pair)
    }
}

// A pair with an empty side is answered here; every other one is appended to the list of its class.
// stat[0 .. 7]: entries of the class lists, [8] sum of |query| |text|, [9] longest query, [10] longest text of the striped class
__global__ __launch_bounds__(SQ_TPB) void k_ix_classify(const sw_infix_pair *__restrict__ pairs, const uint32_t *__restrict__ out_idx, const uint64_t *__restrict__ qoff,
                                                        uint64_t n, uint32_t cap, uint32_t *__restrict__ lists, unsigned long long *__restrict__ stat,
                                                        uint32_t *__restrict__ dist, uint32_t *__restrict__ end)
{
    const uint64_t i = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x;
    const uint32_t lane = threadIdx.x % SQ_WAVE;
    uint32_t cls = IX_CLASSES, m = 0, tn = 0;
    unsigned long long cells = 0;
    if (i < n) {
        const sw_infix_pair p = pairs[i];
        m = (uint32_t)(qoff[p.query + 1] - qoff[p.query]);
        tn = p.stop - p.start;
        cells = (unsigned long long)m * tn;
        if (m == 0 || tn == 0) {
            const uint32_t oi = out_idx ? out_idx[i] : (uint32_t)i;
            dist[oi] = m;         // an empty query: 0; an empty text: the whole query is inserted
            end[oi] = p.start;
        } else {
            const uint32_t nb = (m + 63) >> 6;
            cls = 0;
            if (nb > cap) cls = IX_CLASSES - 1;
            else
                while ((1u << cls) < nb) ++cls;
        }
    }
    for (uint32_t c = 0; c < IX_CLASSES; ++c) {
        const unsigned long long mask = __ballot(cls == c);
        if (!mask) continue;   // (uniform)
        unsigned long long at = 0;
        if (lane == (uint32_t)__ffsll((long long)mask) - 1) at = atomicAdd(stat + c, (unsigned long long)__popcll(mask));
        at = __shfl(at, __ffsll((long long)mask) - 1, SQ_WAVE);
        if (cls == c) lists[(uint64_t)c * n + at + __popcll(mask & ((1ull << lane) - 1))] = (uint32_t)i;
    }
    for (uint32_t d = SQ_WAVE / 2; d; d >>= 1) cells += __shfl_down(cells, d, SQ_WAVE);
    if (lane == 0 && cells) atomicAdd(stat + 8, cells);
    if (m) atomicMax(stat + 9, (unsigned long long)m);
    if (cls == IX_CLASSES - 1) atomicMax(stat + 10, (unsigned long long)tn);
}

}  // namespace

// dist / end of n valid pairs (device list).  counters[6] = { pairs, cells, striped pairs, longest query, launches, block bound }
void infix_device(const Runs &runs, const QueryPack &P, const sw_infix_pair *d_pairs, const uint32_t *d_out_idx, uint64_t n, uint32_t *d_dist, uint32_t *d_end,
                  uint64_t *counters, double *ms_out)
{
    Event e0, e1;
    SW_HIP(hipEventRecord(e0, HIT_STREAM));
    const uint32_t cap = ed_cap_blocks();
    unsigned long long stat[11] = {};
    uint64_t launches = 0;
    if (n) {
        if (n > SQ_MAX_LIST) raise(SW_ERR_VALUE, "infix distances: %llu pairs exceed one launch of the list kernels (%llu)", (unsigned long long)n, (unsigned long long)SQ_MAX_LIST);
        DevArray<uint32_t> lists((uint64_t)IX_CLASSES * n);
        DevArray<unsigned long long> d_stat(11);
        SW_HIP(hipMemsetAsync(d_stat.p, 0, sizeof stat, HIT_STREAM));
        hipLaunchKernelGGL(k_ix_classify, dim3(sq_blocks(n)), dim3(SQ_TPB), 0, HIT_STREAM, d_pairs, d_out_idx, (const uint64_t *)P.off.p, n, cap, lists.p, d_stat.p,
                           d_dist, d_end);
        SW_HIP(hipGetLastError());
        SW_HIP(hipMemcpyAsync(stat, d_stat.p, sizeof stat, hipMemcpyDeviceToHost, HIT_STREAM));
        SW_HIP(hipStreamSynchronize(HIT_STREAM));
        IxArgs a{};
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
        const uint64_t max_threads = (uint64_t)launch_blocks(SQ_BLOCKS_ENV) * SQ_TPB;
        for (uint32_t c = 0; c + 1 < IX_CLASSES; ++c) {   // register route, g = 2^c lanes per pair
            const uint64_t cnt = stat[c], g = 1ull << c, per_launch = std::max<uint64_t>(max_threads / g, 1);
            for (uint64_t x0 = 0; x0 < cnt; x0 += per_launch, ++launches) {
                a.list = lists.p + (uint64_t)c * n + x0;
                a.count = std::min<uint64_t>(per_launch, cnt - x0);
                a.g = (uint32_t)g;
                hipLaunchKernelGGL(k_ix, dim3(sq_blocks(a.count * g)), dim3(SQ_TPB), 0, HIT_STREAM, a);
                SW_HIP(hipGetLastError());
            }
        }
        DevArray<uint8_t> scratch;
        if (const uint64_t cnt = stat[IX_CLASSES - 1]) {   // striped route: the largest power of two <= cap lanes per pair
            uint32_t g = 1;
            while (g * 2 <= cap) g *= 2;
            const uint32_t groups = (uint32_t)std::min<uint64_t>({cnt, (uint64_t)IX_STRIPE_GROUPS, std::max<uint64_t>(max_threads / g, 1)});
            a.carry_stride = ((uint64_t)stat[10] + 15) & ~7ull;
            scratch.alloc((uint64_t)groups * a.carry_stride);
            a.carry = scratch.p;
            a.list = lists.p + (uint64_t)(IX_CLASSES - 1) * n;
            a.count = cnt;
            a.g = g;
            hipLaunchKernelGGL(k_ix_striped, dim3(sq_blocks((uint64_t)groups * g)), dim3(SQ_TPB), 0, HIT_STREAM, a, groups);
            SW_HIP(hipGetLastError());
            ++launches;
        }
        SW_HIP(hipEventRecord(e1, HIT_STREAM));
        SW_HIP(hipStreamSynchronize(HIT_STREAM));   // (lists / scratch go back to the pool behind the kernels)
    } else {
        SW_HIP(hipEventRecord(e1, HIT_STREAM));
        SW_HIP(hipStreamSynchronize(HIT_STREAM));
    }
    if (counters) {
        const uint64_t cn[6] = {n, stat[8], stat[IX_CLASSES - 1], stat[9], launches, cap};
        memcpy(counters, cn, sizeof cn);
    }
    if (ms_out) {
        float ms = 0;
        SW_HIP(hipEventElapsedTime(&ms, e0, e1));
        ms_out[0] = ms;
    }
}

namespace {

// ---- Layer B: seeds -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCR_TPB) void k_hit_mult(uint64_t base, uint64_t end, const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ number,
                                                      uint32_t *__restrict__ mult)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j < end) atomicAdd(mult + number[sidx[j]], 1u);
}

// valid window j whose word no other window has and that is not its own reverse complement: the seed of its word's number
__global__ __launch_bounds__(SCR_TPB) void k_hit_seeds(uint64_t base, uint64_t end, const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ number,
                                                       const uint32_t *__restrict__ mult, const uint64_t *__restrict__ by_number, const uint32_t *__restrict__ vpos,
                                                       const uint8_t *__restrict__ text, const uint64_t *__restrict__ off, uint32_t nq, uint32_t k,
                                                       uint32_t *__restrict__ seed_q, uint32_t *__restrict__ seed_i, uint8_t *__restrict__ seed_fc,
                                                       uint32_t *__restrict__ n_seeds)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j >= end) return;
    const uint32_t id = number[sidx[j]];
    if (mult[id] != 1) return;
    const uint64_t word = by_number[id];
    uint64_t rc = 0, x = word, fwd = 0;
    const uint64_t pos = vpos[j];
    for (uint32_t i = 0; i < k; ++i) {
        rc = (rc << 2) | (3 - (x & 3));
        x >>= 2;
        fwd = (fwd << 2) | (uint64_t)(base_code(text[pos + i]) & 3u);
    }
    if (rc == word) return;   // its own reverse complement: the orientation of a hit would be undefined
    const uint32_t q = query_of(off, nq, pos);
    seed_q[id] = q;
    seed_i[id] = (uint32_t)(pos - off[q]);
    seed_fc[id] = fwd == word ? 1 : 0;
    atomicAdd(n_seeds + q, 1u);
}

// ---- Layer B: shared seeds -----------------------------------------------------------------------------
// A word that 1 .. c windows of all query text have, and that is not its own reverse complement, is a seed that every one of those
// windows owns.  Both routes count what that rule keeps and drops (sw_hits_seed_stats); the unique route is the rule at c = 1.
enum { SS_WORDS, SS_OCC, SS_DROPPED_WORDS, SS_DROPPED_OCC, SS_PALINDROMES, SS_LONGEST, SS_N };

__device__ __forceinline__ bool own_revcomp(uint64_t word, uint32_t k)
{
    uint64_t rc = 0, x = word;
    for (uint32_t i = 0; i < k; ++i) {
        rc = (rc << 2) | (3 - (x & 3));
        x >>= 2;
    }
    return rc == word;
}

// distinct word id: kept[id] = its windows if it is a seed under the cap c, else 0 (kept == nullptr: only the counts are taken).
// A palindromic word counts as that, whatever its windows; a dropped word is a non-palindromic one above the cap
__global__ __launch_bounds__(SCR_TPB) void k_hit_keep(uint64_t base, uint64_t end, const uint32_t *__restrict__ mult, const uint64_t *__restrict__ by_number, uint32_t k,
                                                      uint32_t c, uint32_t *__restrict__ kept, unsigned long long *__restrict__ stat)
{
    const uint64_t id = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    uint32_t m = 0, keep = 0, pal = 0;
    if (id < end) {
        m = mult[id];
        pal = own_revcomp(by_number[id], k) ? 1u : 0u;
        keep = (!pal && m <= c) ? m : 0u;
        if (kept) kept[id] = keep;
    }
    const uint32_t dropped = (!pal && m > c) ? m : 0u;
    const unsigned long long words = wave_sum(keep ? 1 : 0), occ = wave_sum(keep), d_words = wave_sum(dropped ? 1 : 0), d_occ = wave_sum(dropped),
                             pals = wave_sum(pal);
    const uint32_t longest = wave_max(keep);
    if (threadIdx.x % SCR_WAVE == 0) {
        if (words) atomicAdd(stat + SS_WORDS, words);
        if (occ) atomicAdd(stat + SS_OCC, occ);
        if (d_words) atomicAdd(stat + SS_DROPPED_WORDS, d_words);
        if (d_occ) atomicAdd(stat + SS_DROPPED_OCC, d_occ);
        if (pals) atomicAdd(stat + SS_PALINDROMES, pals);
        if (longest) atomicMax(stat + SS_LONGEST, (unsigned long long)longest);
    }
}

struct KeptAt {
    const uint32_t *c;
    uint64_t n;
    __host__ __device__ uint32_t operator()(uint64_t i) const { return i < n ? c[i] : 0u; }
};

// valid window j as (its word's number << 32 | j): sorted, a word's windows lie together in text order
__global__ __launch_bounds__(SCR_TPB) void k_own_keys(uint64_t base, uint64_t end, const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ number,
                                                      uint64_t *__restrict__ okey)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j < end) okey[j] = ((uint64_t)number[sidx[j]] << 32) | j;
}

// An owner record: window-is-canonical << 63 | query << 32 | offset in the query (a query index takes 31 bits here).
// Placement: entry s of the sorted (number, window) keys is the owner of rank (s - the first entry of its number) in its word's
// list, so a list holds its windows in text order -- no atomic decides a place.  The rank is counted backwards over at most c - 1
// entries.  n_seeds counts the owners of every query (integer adds: the sum does not depend on their order)
__global__ __launch_bounds__(SCR_TPB) void k_own_fill(uint64_t base, uint64_t end, const uint64_t *__restrict__ okey, const uint32_t *__restrict__ kept,
                                                      const uint32_t *__restrict__ occ_off, const uint64_t *__restrict__ by_number, const uint32_t *__restrict__ vpos,
                                                      const uint8_t *__restrict__ text, const uint64_t *__restrict__ off, uint32_t nq, uint32_t k,
                                                      uint64_t *__restrict__ owners, uint32_t *__restrict__ n_seeds)
{
    const uint64_t s = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (s >= end) return;
    const uint64_t x = okey[s];
    const uint32_t id = (uint32_t)(x >> 32), j = (uint32_t)x;
    if (!kept[id]) return;
    uint32_t rank = 0;
    while (rank < s && (uint32_t)(okey[s - rank - 1] >> 32) == id) ++rank;   // (< kept[id] <= c)
    const uint64_t pos = vpos[j], word = by_number[id];
    uint64_t fwd = 0;
    for (uint32_t i = 0; i < k; ++i) fwd = (fwd << 2) | (uint64_t)(base_code(text[pos + i]) & 3u);
    const uint32_t q = query_of(off, nq, pos);
    owners[occ_off[id] + rank] = (fwd == word ? 1ull << 63 : 0ull) | ((uint64_t)q << 32) | (pos - off[q]);
    atomicAdd(n_seeds + q, 1u);
}

// ---- Layer B: probe -------------------------------------------------------------------------------------------------------------
struct HitArgs {
    RunView v;                       // with run_rec / run_pos
    Table t;
    const uint32_t *seed_q, *seed_i;
    const uint8_t *seed_fc;
    const uint64_t *qoff;
    uint64_t *buf;
    uint64_t cap;                    // keys the buffer holds
    unsigned long long *cursor;      // keys appended (above cap: the chunk overflowed and nothing more is written)
    uint32_t k, band_bits, rec_bits;
};

__global__ __launch_bounds__(SCR_TPB) void k_hit_probe(HitArgs g)
{
    if (*(volatile unsigned long long *)g.cursor > g.cap) return;   // (the whole wave: the chunk has overflowed, it is redone anyway)
    const uint32_t lane = threadIdx.x % SCR_WAVE;
    uint32_t r, n_mine;
    uint64_t first;
    if (!wave_tile(g.v, lane, r, first, n_mine)) return;   // (the whole wave)
    const uint32_t k = g.k;
    uint64_t key[SCR_L];
    uint32_t have = 0, cnt = 0;         // bit j: key[j] is a hit
    KmerRoller R(g.v.packed, k);
    if (n_mine) {
        R.start(g.v.run_base[r] + first);
        for (uint32_t i = 0; i + 1 < k; ++i) R.roll();
        uint64_t canon[SCR_L];
        uint32_t home[SCR_L], slot[SCR_L], is_fwd = 0;
#pragma unroll
        for (uint32_t j = 0; j < SCR_L; ++j) {
            canon[j] = 0;
            if (j < n_mine) {
                R.roll();
                canon[j] = R.fwd < R.rev ? R.fwd : R.rev;
                is_fwd |= (R.fwd < R.rev ? 1u : 0u) << j;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < SCR_L; ++j) {   // the 16 first-slot loads leave together
            home[j] = scr_home(canon[j], g.t.bits);
            slot[j] = j < n_mine ? g.t.slots[home[j]] : 0u;
        }
        const uint32_t rec = g.v.run_rec[r];
        const uint64_t p0 = (uint64_t)g.v.run_pos[r] + first;
#pragma unroll
        for (uint32_t j = 0; j < SCR_L; ++j) {
            key[j] = 0;
            if (!slot[j]) continue;
            const uint32_t id = scr_find_from(g.t, canon[j], home[j], slot[j]);
            if (id == SCR_NONE) continue;
            const uint32_t q = g.seed_q[id];
            if (q == SCR_NONE) continue;
            const uint64_t m = g.qoff[q + 1] - g.qoff[q], i = g.seed_i[id];
            const uint32_t o = (((is_fwd >> j) & 1u) != (uint32_t)g.seed_fc[id]) ? 1u : 0u;
            const uint64_t io = o ? m - k - i : i, e = p0 + j + (m - k) - io;   // (m - k - io >= 0)
            key[j] = ((((uint64_t)q << g.rec_bits | rec) << 1 | o) << g.band_bits) | (e >> HIT_BAND_SHIFT);
            have |= 1u << j;
            ++cnt;
        }
    }
    const WaveRange w = wave_append(g.cursor, lane, cnt);   // one atomic on the cursor per wave
    if (!w.total) return;                             // (uniform)
    if (w.base + w.total > g.cap) return;             // (uniform) overflow: the host reads it from the cursor
    unsigned long long at = w.base + w.offset;
#pragma unroll
    for (uint32_t j = 0; j < SCR_L; ++j)
        if ((have >> j) & 1u) g.buf[at++] = key[j];
}

// The shared-seed probe: k_hit_probe's walk, loads and keys, but a window's word has a list of owners and yields a key per owner.
// Two steps: the lane's 16 ids are resolved to (first owner, owners) and the owners summed -- one wave_append with the sum, the
// overflow rule as above --, then the lists are walked and the keys stored.  The loop over the 16 windows is unrolled both times, so
// beg / len are registers (no array is indexed by a run-time value); the loop over a list has a run-time length and indexes nothing.
struct HitSharedArgs {
    RunView v;                       // with run_rec / run_pos
    Table t;
    const uint32_t *occ_off;         // [distinct words + 1]: word id's owners are owners[occ_off[id] .. occ_off[id + 1])
    const uint64_t *owners;          // window-is-canonical << 63 | query << 32 | offset
    const uint64_t *qoff;
    uint64_t *buf;
    uint64_t cap;
    unsigned long long *cursor;
    uint32_t k, band_bits, rec_bits;
};

__global__ __launch_bounds__(SCR_TPB) void k_hit_probe_shared(HitSharedArgs g)
{
    if (*(volatile unsigned long long *)g.cursor > g.cap) return;   // (the whole wave: the chunk has overflowed, it is redone anyway)
    const uint32_t lane = threadIdx.x % SCR_WAVE;
    uint32_t r, n_mine;
    uint64_t first;
    if (!wave_tile(g.v, lane, r, first, n_mine)) return;   // (the whole wave)
    const uint32_t k = g.k;
    uint32_t beg[SCR_L], len[SCR_L], is_fwd = 0, cnt = 0, rec = 0;
    uint64_t p0 = 0;
#pragma unroll
    for (uint32_t j = 0; j < SCR_L; ++j) beg[j] = len[j] = 0;
    if (n_mine) {
        KmerRoller R(g.v.packed, k);
        R.start(g.v.run_base[r] + first);
        for (uint32_t i = 0; i + 1 < k; ++i) R.roll();
        uint64_t canon[SCR_L];
        uint32_t home[SCR_L], slot[SCR_L];
#pragma unroll
        for (uint32_t j = 0; j < SCR_L; ++j) {
            canon[j] = 0;
            if (j < n_mine) {
                R.roll();
                canon[j] = R.fwd < R.rev ? R.fwd : R.rev;
                is_fwd |= (R.fwd < R.rev ? 1u : 0u) << j;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < SCR_L; ++j) {   // the 16 first-slot loads leave together
            home[j] = scr_home(canon[j], g.t.bits);
            slot[j] = j < n_mine ? g.t.slots[home[j]] : 0u;
        }
        rec = g.v.run_rec[r];
        p0 = (uint64_t)g.v.run_pos[r] + first;
#pragma unroll
        for (uint32_t j = 0; j < SCR_L; ++j) {
            if (!slot[j]) continue;
            const uint32_t id = scr_find_from(g.t, canon[j], home[j], slot[j]);
            if (id == SCR_NONE) continue;
            beg[j] = g.occ_off[id];
            len[j] = g.occ_off[id + 1] - beg[j];   // (0: the word is no seed)
            cnt += len[j];                         // (<= 16 * 256)
        }
    }
    const WaveRange w = wave_append(g.cursor, lane, cnt);   // one atomic on the cursor per wave
    if (!w.total) return;                             // (uniform)
    if (w.base + w.total > g.cap) return;             // (uniform) overflow: the host reads it from the cursor
    unsigned long long at = w.base + w.offset;        // the lane writes [at, at + cnt), inside the wave's range
#pragma unroll
    for (uint32_t j = 0; j < SCR_L; ++j)
        for (uint32_t x = 0; x < len[j]; ++x) {
            const uint64_t own = g.owners[beg[j] + x];
            const uint32_t q = (uint32_t)(own >> 32) & 0x7FFFFFFFu;
            const uint64_t m = g.qoff[q + 1] - g.qoff[q], i = own & 0xFFFFFFFFull;
            const uint32_t o = (((is_fwd >> j) & 1u) != (uint32_t)(own >> 63)) ? 1u : 0u;
            const uint64_t io = o ? m - k - i : i, e = p0 + j + (m - k) - io;   // (m - k - io >= 0)
            g.buf[at++] = ((((uint64_t)q << g.rec_bits | rec) << 1 | o) << g.band_bits) | (e >> HIT_BAND_SHIFT);
        }
}

// ---- Layer B: vote --------------------------------------------------------------------------------------------------------------
// run r of the sorted keys: score = its length + the length of the run of the next band, if that is the next run.  The winner of a
// (query, assembly): the largest (score, ~r) -- the runs ascend by (record, orientation, band) inside the pair
__global__ __launch_bounds__(SCR_TPB) void k_hit_vote(uint64_t base, uint64_t end, const uint64_t *__restrict__ ukey, const uint32_t *__restrict__ upos, uint64_t n_keys,
                                                      const uint32_t *__restrict__ rec_asm, uint32_t band_bits, uint32_t rec_bits, uint32_t asm0, uint32_t rows,
                                                      unsigned long long *__restrict__ best)
{
    const uint64_t r = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (r >= end) return;
    const uint64_t n_runs = end, key = ukey[r];   // (launched over all runs in one range or several: `end` of the last is n_runs)
    const uint64_t next = r + 1 < n_runs ? upos[r + 1] : n_keys;
    uint64_t score = next - upos[r];
    if (r + 1 < n_runs && ukey[r + 1] == key + 1) score += (r + 2 < n_runs ? upos[r + 2] : n_keys) - next;
    const uint32_t rec = (uint32_t)((key >> (band_bits + 1)) & ((1ull << rec_bits) - 1));
    const uint64_t q = key >> (band_bits + 1 + rec_bits);
    atomicMax(best + q * rows + (rec_asm[rec] - asm0), (unsigned long long)(score << 32 | (0xFFFFFFFFull - r)));
}

// cell (query, assembly of the chunk) with a winner: its fields, and its window as a pair of Layer A
__global__ __launch_bounds__(SCR_TPB) void k_hit_finish(uint64_t base, uint64_t end, const unsigned long long *__restrict__ best, const uint64_t *__restrict__ ukey,
                                                        const uint64_t *__restrict__ qoff, const uint32_t *__restrict__ rec_len, uint32_t k, uint32_t band_bits,
                                                        uint32_t rec_bits, uint32_t asm0, uint32_t rows, uint64_t n_asm, uint32_t *__restrict__ seeds,
                                                        uint32_t *__restrict__ record, uint32_t *__restrict__ strand, sw_infix_pair *__restrict__ pairs,
                                                        uint32_t *__restrict__ out_idx, uint32_t *__restrict__ n_pairs)
{
    const uint64_t c = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (c >= end) return;
    const unsigned long long v = best[c];
    if (!v) return;
    const uint64_t q = c / rows, a = asm0 + c % rows, cell = q * n_asm + a;
    const uint64_t key = ukey[0xFFFFFFFFull - (v & 0xFFFFFFFFull)];
    const uint64_t band = key & ((1ull << band_bits) - 1);
    const uint32_t o = (uint32_t)(key >> band_bits) & 1u, rec = (uint32_t)((key >> (band_bits + 1)) & ((1ull << rec_bits) - 1));
    seeds[cell] = (uint32_t)(v >> 32);
    record[cell] = rec;
    strand[cell] = o;
    const long long m = (long long)(qoff[q + 1] - qoff[q]), s0 = (long long)(band << HIT_BAND_SHIFT) - (m - (long long)k);
    const long long lo = s0 - 64 > 0 ? s0 - 64 : 0, len = rec_len[rec], hi = s0 + 192 + m < len ? s0 + 192 + m : len;
    const uint32_t at = atomicAdd(n_pairs, 1u);
    pairs[at] = sw_infix_pair{(uint32_t)q, o, rec, (uint32_t)lo, (uint32_t)hi};
    out_idx[at] = (uint32_t)cell;
}

// ---- Layer B: every locus ------------------------------------------------------------------------------
enum { LF_QUERY, LF_ASM, LF_RECORD, LF_STRAND, LF_BAND, LF_SEEDS, LF_DIST, LF_END, LF_START, LF_NIDENT, LF_MISMATCH, LF_GAPS, LF_DUP };
constexpr int LF_CHUNK = LF_DUP;   // what a chunk's list holds: everything but dup, which only the final order defines

struct LociPtrs {
    uint32_t *f[LF_CHUNK];
};

// the score of run r as k_hit_vote computes it
__device__ __forceinline__ uint64_t run_score(const uint64_t *__restrict__ ukey, const uint32_t *__restrict__ upos, uint64_t n_runs, uint64_t n_keys, uint64_t r)
{
    const uint64_t next = r + 1 < n_runs ? upos[r + 1] : n_keys;
    uint64_t score = next - upos[r];
    if (r + 1 < n_runs && ukey[r + 1] == ukey[r] + 1) score += (r + 2 < n_runs ? upos[r + 2] : n_keys) - next;
    return score;
}

// run r is a locus: its score reaches min_seeds, and no run of the same (query, record, orientation) within two bands beats it -- a
// larger score, or the same score in a smaller band.  The keys are distinct and sorted, so such a run lies within two places; the
// fields are compared, not key +- 2 (the band field is one value wider than the largest band: b + 2 may carry)
__global__ __launch_bounds__(SCR_TPB) void k_hit_peaks(uint64_t base, uint64_t end, const uint64_t *__restrict__ ukey, const uint32_t *__restrict__ upos, uint64_t n_runs,
                                                       uint64_t n_keys, uint32_t band_bits, uint64_t min_seeds, uint8_t *__restrict__ flag)
{
    const uint64_t r = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (r >= end) return;
    const uint64_t mask = (1ull << band_bits) - 1, key = ukey[r], grp = key >> band_bits, band = key & mask;
    const uint64_t s = run_score(ukey, upos, n_runs, n_keys, r);
    bool locus = s >= min_seeds;
    for (uint64_t d = 1; d <= 2 && locus; ++d) {
        if (r >= d) {
            const uint64_t y = ukey[r - d];
            if ((y >> band_bits) == grp && band - (y & mask) <= 2 && run_score(ukey, upos, n_runs, n_keys, r - d) >= s) locus = false;
        }
        if (r + d < n_runs) {
            const uint64_t y = ukey[r + d];
            if ((y >> band_bits) == grp && (y & mask) - band <= 2 && run_score(ukey, upos, n_runs, n_keys, r + d) > s) locus = false;
        }
    }
    flag[r] = locus ? 1 : 0;
}

// flagged run r is entry at[r] of the chunk's list: its fields, and its window as a pair of Layer A
__global__ __launch_bounds__(SCR_TPB) void k_hit_loci(uint64_t base, uint64_t end, const uint8_t *__restrict__ flag, const uint32_t *__restrict__ at,
                                                      const uint64_t *__restrict__ ukey, const uint32_t *__restrict__ upos, uint64_t n_runs, uint64_t n_keys,
                                                      const uint64_t *__restrict__ qoff, const uint32_t *__restrict__ rec_len, const uint32_t *__restrict__ rec_asm,
                                                      uint32_t k, uint32_t band_bits, uint32_t rec_bits, LociPtrs out, sw_infix_pair *__restrict__ pairs)
{
    const uint64_t r = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (r >= end || !flag[r]) return;
    const uint32_t j = at[r];
    const uint64_t key = ukey[r], band = key & ((1ull << band_bits) - 1), q = key >> (band_bits + 1 + rec_bits);
    const uint32_t o = (uint32_t)(key >> band_bits) & 1u, rec = (uint32_t)((key >> (band_bits + 1)) & ((1ull << rec_bits) - 1));
    out.f[LF_QUERY][j] = (uint32_t)q;
    out.f[LF_ASM][j] = rec_asm[rec];
    out.f[LF_RECORD][j] = rec;
    out.f[LF_STRAND][j] = o;
    out.f[LF_BAND][j] = (uint32_t)band;
    out.f[LF_SEEDS][j] = (uint32_t)run_score(ukey, upos, n_runs, n_keys, r);
    const long long m = (long long)(qoff[q + 1] - qoff[q]), s0 = (long long)(band << HIT_BAND_SHIFT) - (m - (long long)k);
    const long long lo = s0 - 64 > 0 ? s0 - 64 : 0, len = rec_len[rec], hi = s0 + 192 + m < len ? s0 + 192 + m : len;
    pairs[j] = sw_infix_pair{(uint32_t)q, o, rec, (uint32_t)lo, (uint32_t)hi};
}

// entry j of a chunk's list is entry g0 + j of all chunks' lists, one behind the other.  A cell's entries are contiguous there (an
// assembly belongs to one chunk): the first one writes first[cell], the last one past[cell]
__global__ __launch_bounds__(SCR_TPB) void k_loci_bounds(uint64_t base, uint64_t end, const uint32_t *__restrict__ query, const uint32_t *__restrict__ assembly,
                                                         uint64_t n, uint64_t g0, uint64_t n_asm, uint64_t *__restrict__ first, uint64_t *__restrict__ past)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j >= end) return;
    const uint64_t cell = query[j] * n_asm + assembly[j];
    if (j == 0 || query[j - 1] * n_asm + assembly[j - 1] != cell) first[cell] = g0 + j;
    if (j + 1 == n || query[j + 1] * n_asm + assembly[j + 1] != cell) past[cell] = g0 + j + 1;
}

// the local alignment's nine columns of a chunk's entries, to the place k_loci_gather gave the entry
struct LocalPtrs {
    uint32_t *f[LOCAL_FIELDS];
};
__global__ __launch_bounds__(SCR_TPB) void k_loci_gather_local(uint64_t base, uint64_t end, const uint32_t *__restrict__ query, const uint32_t *__restrict__ assembly,
                                                               LocalPtrs in, uint64_t g0, uint64_t n_asm, const uint64_t *__restrict__ first,
                                                               const uint64_t *__restrict__ cell_off, LocalPtrs out)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j >= end) return;
    const uint64_t cell = query[j] * n_asm + assembly[j], dst = cell_off[cell] + (g0 + j - first[cell]);
#pragma unroll
    for (uint32_t f = 0; f < LOCAL_FIELDS; ++f) out.f[f][dst] = in.f[f][j];
}

struct CellCount {
    const uint64_t *first, *past;
    uint64_t n;
    __host__ __device__ uint64_t operator()(uint64_t c) const { return c < n ? past[c] - first[c] : 0ull; }
};

// a chunk's entries to their place in the final order: the cell's offset + the entry's rank inside its cell
__global__ __launch_bounds__(SCR_TPB) void k_loci_gather(uint64_t base, uint64_t end, LociPtrs in, uint64_t g0, uint64_t n_asm, const uint64_t *__restrict__ first,
                                                         const uint64_t *__restrict__ cell_off, LociPtrs out)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j >= end) return;
    const uint64_t cell = in.f[LF_QUERY][j] * n_asm + in.f[LF_ASM][j], dst = cell_off[cell] + (g0 + j - first[cell]);
#pragma unroll
    for (int f = 0; f < LF_CHUNK; ++f) out.f[f][dst] = in.f[f][j];
}

// locus j repeats its predecessor: the same query, record, strand, start and end -- two windows found one copy
__global__ __launch_bounds__(SCR_TPB) void k_hit_dups(uint64_t base, uint64_t end, LociPtrs l, uint32_t *__restrict__ dup)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j >= end) return;
    const bool same = j > 0 && l.f[LF_QUERY][j] == l.f[LF_QUERY][j - 1] && l.f[LF_RECORD][j] == l.f[LF_RECORD][j - 1] &&
                      l.f[LF_STRAND][j] == l.f[LF_STRAND][j - 1] && l.f[LF_START][j] == l.f[LF_START][j - 1] && l.f[LF_END][j] == l.f[LF_END][j - 1];
    dup[j] = same ? 1u : 0u;
}

// a thread per cell over its contiguous segment: no atomics, so nothing depends on an order
__global__ __launch_bounds__(SCR_TPB) void k_loci_reduce(uint64_t base, uint64_t end, const uint64_t *__restrict__ cell_off, const uint32_t *__restrict__ dup,
                                                         const uint32_t *__restrict__ nident, uint32_t *__restrict__ n_loci, uint32_t *__restrict__ sum_nident)
{
    const uint64_t c = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (c >= end) return;
    uint32_t n = 0, s = 0;
    for (uint64_t j = cell_off[c]; j < cell_off[c + 1]; ++j)
        if (!dup[j]) {
            ++n;
            s += nident[j];
        }
    n_loci[c] = n;
    sum_nident[c] = s;
}

struct LociChunk {
    uint64_t n = 0;
    DevArray<uint32_t> f[LF_CHUNK];
    DevArray<uint32_t> lf[LOCAL_FIELDS];   // the local alignment's figures (allocated with a scoring system only)
    LociPtrs ptrs() const
    {
        LociPtrs p;
        for (int i = 0; i < LF_CHUNK; ++i) p.f[i] = f[i].p;
        return p;
    }
};

struct AsU64 {
    __host__ __device__ uint64_t operator()(uint32_t x) const { return x; }
};

// the chunks' lists into the final order (query, assembly, record, orientation, band), duplicates, and the per-cell reduction
void finish_loci(std::vector<LociChunk> &chunks, uint64_t nq, uint64_t n_asm, uint64_t max_q, hipStream_t stream, HitLoci &L, bool local)
{
    const uint64_t n_cells = nq * n_asm;
    uint64_t total = 0;
    for (const LociChunk &c : chunks) total += c.n;
    L.n = total;
    L.cell_off.alloc(n_cells + 1);
    L.n_loci.alloc(n_cells);
    L.sum_nident.alloc(n_cells);
    for (int f = 0; f < LOCI_LIST_FIELDS; ++f) L.f[f].alloc(total);
    if (local)
        for (uint32_t f = 0; f < LOCAL_FIELDS; ++f) L.lf[f].alloc(total);
    if (!total) {
        SW_HIP(hipMemsetAsync(L.cell_off.p, 0, (n_cells + 1) * 8, stream));
        if (n_cells) {
            SW_HIP(hipMemsetAsync(L.n_loci.p, 0, n_cells * 4, stream));
            SW_HIP(hipMemsetAsync(L.sum_nident.p, 0, n_cells * 4, stream));
        }
        SW_HIP(hipStreamSynchronize(stream));
        return;
    }
    DevArray<uint64_t> first(n_cells), past(n_cells);
    SW_HIP(hipMemsetAsync(first.p, 0, n_cells * 8, stream));
    SW_HIP(hipMemsetAsync(past.p, 0, n_cells * 8, stream));
    uint64_t g0 = 0;
    for (const LociChunk &c : chunks) {
        launch_1d(k_loci_bounds, c.n, stream, (const uint32_t *)c.f[LF_QUERY].p, (const uint32_t *)c.f[LF_ASM].p, c.n, g0, n_asm, first.p, past.p);
        g0 += c.n;
    }
    {
        size_t tmp_bytes = 0;
        auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), CellCount{first.p, past.p, n_cells});
        SW_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, in, L.cell_off.p, uint64_t(0), n_cells + 1, rocprim::plus<uint64_t>(), stream));
        DevArray<unsigned char> tmp(tmp_bytes);
        SW_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, in, L.cell_off.p, uint64_t(0), n_cells + 1, rocprim::plus<uint64_t>(), stream));
        SW_HIP(hipStreamSynchronize(stream));
    }
    LociPtrs out;
    for (int f = 0; f < LF_CHUNK; ++f) out.f[f] = L.f[f].p;
    g0 = 0;
    for (LociChunk &c : chunks) {
        launch_1d(k_loci_gather, c.n, stream, c.ptrs(), g0, n_asm, (const uint64_t *)first.p, (const uint64_t *)L.cell_off.p, out);
        if (local) {
            LocalPtrs lin, lout;
            for (uint32_t f = 0; f < LOCAL_FIELDS; ++f) {
                lin.f[f] = c.lf[f].p;
                lout.f[f] = L.lf[f].p;
            }
            launch_1d(k_loci_gather_local, c.n, stream, (const uint32_t *)c.f[LF_QUERY].p, (const uint32_t *)c.f[LF_ASM].p, lin, g0, n_asm, (const uint64_t *)first.p,
                      (const uint64_t *)L.cell_off.p, lout);
        }
        g0 += c.n;
    }
    launch_1d(k_hit_dups, total, stream, out, L.f[LF_DUP].p);
    launch_1d(k_loci_reduce, n_cells, stream, (const uint64_t *)L.cell_off.p, (const uint32_t *)L.f[LF_DUP].p, (const uint32_t *)L.f[LF_NIDENT].p, L.n_loci.p,
              L.sum_nident.p);
    // the largest cell and the loci that are no duplicates
    DevArray<uint64_t> d_red(2);
    uint64_t red[2] = {};
    {
        size_t tmp_bytes = 0;
        auto in = rocprim::make_transform_iterator((const uint32_t *)L.n_loci.p, AsU64{});
        SW_HIP(rocprim::reduce(nullptr, tmp_bytes, in, d_red.p, uint64_t(0), n_cells, rocprim::maximum<uint64_t>(), stream));
        DevArray<unsigned char> tmp(tmp_bytes);
        SW_HIP(rocprim::reduce(tmp.p, tmp_bytes, in, d_red.p, uint64_t(0), n_cells, rocprim::maximum<uint64_t>(), stream));
        SW_HIP(rocprim::reduce(tmp.p, tmp_bytes, in, d_red.p + 1, uint64_t(0), n_cells, rocprim::plus<uint64_t>(), stream));
        SW_HIP(hipMemcpyAsync(red, d_red.p, 16, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));   // (the chunks' lists and the scratch are read until here)
    }
    L.max_per_cell = red[0];
    L.n_dup = total - red[1];
    if (L.max_per_cell * max_q >= (1ull << 32))
        raise(SW_ERR_VALUE, "best hits: %llu loci in one cell times the longest query (%llu) do not fit the 32-bit sum of nident", (unsigned long long)L.max_per_cell,
              (unsigned long long)max_q);
}

}  // namespace
}  // namespace sw

namespace sw {
namespace {

// align: the traceback of every chunk's winners (align.hip) right behind their distances, while the chunk's windows exist.
// min_seeds > 0: the loci mode (it implies align) -- behind the winners of a chunk, every locus of the chunk's runs is listed,
// measured and traced the same way; after the last chunk the lists are ordered and reduced per cell (finish_loci)
// seed_copies: 0 -- the unique-seed route (seed_q / seed_i / seed_fc, k_hit_probe); 1 .. 256 -- the cap of the shared-seed route (owner
// lists, k_hit_probe_shared).  Everything behind the probe is the same code for both
// local != nullptr: the local alignment (local.hip) of the winners' pairs, and in loci mode of the loci's,
// right behind their distances; nullptr: not one pass more than before
// pile != nullptr (it needs align): the winners' traceback also adds every piled winner to the pileup's tables (align.hip, DESIGN.md
// section 3.2k), labelled by its assembly; the loci's traceback stays the plain one
// pile->lengths != nullptr: the winners' traceback is the window walk, which also classes every window of those lengths (DESIGN.md
// section 3.2l)
struct PileCall {
    sw_pileup *p;
    const uint8_t *assembly_group;
    uint64_t n_groups, max_dist_permille;
    sw_windows *w = nullptr;
    const uint32_t *lengths = nullptr;
    uint64_t n_lengths = 0, max_mismatch = 0, three_prime = 0;
};

void batch_best_hits(const sw_batch &b, const uint64_t *offsets, const char *blob, uint64_t nq, uint32_t k, bool align, uint64_t min_seeds, uint32_t seed_copies,
                     const sw_scoring *local, sw_hits &o, const PileCall *pile = nullptr)
{
    const bool loci = min_seeds > 0;
    std::vector<LociChunk> loci_chunks;
    const hipStream_t stream = HIT_STREAM;
    const HostBatch &h = b.host;
    const uint64_t n_asm = h.n_assemblies, n_cells = nq * n_asm;
    if (n_cells >= 0xFFFFFFFFull) raise(SW_ERR_VALUE, "best hits: %llu queries x %llu assemblies exceed 32-bit cell indices", (unsigned long long)nq, (unsigned long long)n_asm);
    o.nq = nq;
    o.n_asm = n_asm;
    o.k = k;
    o.n_seeds.assign(nq, 0);
    for (int f = 0; f < 5; ++f) {
        o.field[f].alloc(n_cells);
        if (n_cells) SW_HIP(hipMemsetAsync(o.field[f].p, (f == 0 || f == 2) ? 0 : 0xFF, n_cells * 4, stream));
    }
    o.aligned = align;
    o.has_loci = loci;
    o.loci.min_seeds = min_seeds;
    if (align)
        for (int f = 0; f < 4; ++f) {
            o.afield[f].alloc(n_cells);
            if (n_cells) SW_HIP(hipMemsetAsync(o.afield[f].p, 0xFF, n_cells * 4, stream));
        }
    if (pile) {
        const uint64_t no_query[1] = {0};
        pile_begin(*pile->p, b.device, nq ? offsets : no_query, nq, pile->n_groups, pile->max_dist_permille, pile->assembly_group, n_asm, n_asm);
        if (pile->w)
            win_begin(*pile->w, b.device, nq ? offsets : no_query, nq, pile->n_groups, pile->lengths, pile->n_lengths, pile->max_mismatch, pile->three_prime);
    }
    o.has_local = local != nullptr;
    if (local)
        for (uint32_t f = 0; f < LOCAL_FIELDS; ++f) {
            o.lfield[f].alloc(n_cells);
            if (n_cells) SW_HIP(hipMemsetAsync(o.lfield[f].p, 0xFF, n_cells * 4, stream));
        }
    // the key's fields: query | record | orientation | band, the band field one value wider than the largest band (b + 1 is looked at)
    uint64_t max_q = 0, max_rec = 0;
    for (uint64_t q = 0; q < nq; ++q) max_q = std::max(max_q, offsets[q + 1] - offsets[q]);
    for (uint32_t l : h.rec_len) max_rec = std::max<uint64_t>(max_rec, l);
    const uint32_t band_bits = bits_of(((max_rec + max_q) >> HIT_BAND_SHIFT) + 1), rec_bits = bits_of(h.rec_len.size() ? h.rec_len.size() - 1 : 0),
                   q_bits = bits_of(nq ? nq - 1 : 0), key_bits = band_bits + 1 + rec_bits + q_bits;
    if (key_bits > 64)
        raise(SW_ERR_VALUE, "best hits: a hit key of %u bits (%u query, %u record, 1 orientation, %u band) does not fit 64", key_bits, q_bits, rec_bits, band_bits);
    Event e0, e1;
    SW_HIP(hipEventRecord(e0, stream));

    // ---- query side: the screen's, then multiplicities and the seed table; the packed queries of Layer A ----
    QuerySide Q;
    build_query_side(offsets, blob, nq, k, stream, Q);
    QueryPack P;
    DevArray<uint32_t> seed_q, seed_i, occ_off;
    DevArray<uint8_t> seed_fc;
    DevArray<uint64_t> owners;
    uint64_t n_seeds_total = 0;
    unsigned long long seed_stat[SS_N] = {};
    const bool shared = seed_copies > 0;
    if (shared && nq > (1ull << 31))
        raise(SW_ERR_VALUE, "best hits: %llu queries exceed the 31 bits an owner record of the shared seeds has for a query", (unsigned long long)nq);
    if (Q.n_distinct) {
        DevArray<uint32_t> mult(Q.n_distinct), d_ns(nq);
        DevArray<unsigned long long> d_stat(SS_N);
        SW_HIP(hipMemsetAsync(mult.p, 0, Q.n_distinct * 4, stream));
        SW_HIP(hipMemsetAsync(d_ns.p, 0, nq * 4, stream));
        SW_HIP(hipMemsetAsync(d_stat.p, 0, sizeof seed_stat, stream));
        launch_1d(k_hit_mult, Q.n_valid, stream, (const uint32_t *)Q.sidx.p, (const uint32_t *)Q.number.p, mult.p);
        if (!shared) {
            seed_q.alloc(Q.n_distinct);
            seed_i.alloc(Q.n_distinct);
            seed_fc.alloc(Q.n_distinct);
            SW_HIP(hipMemsetAsync(seed_q.p, 0xFF, Q.n_distinct * 4, stream));
            SW_HIP(hipMemsetAsync(seed_i.p, 0, Q.n_distinct * 4, stream));
            SW_HIP(hipMemsetAsync(seed_fc.p, 0, Q.n_distinct, stream));
            launch_1d(k_hit_seeds, Q.n_valid, stream, (const uint32_t *)Q.sidx.p, (const uint32_t *)Q.number.p, (const uint32_t *)mult.p, (const uint64_t *)Q.by_number.p,
                      (const uint32_t *)Q.vpos.p, (const uint8_t *)Q.text.p, (const uint64_t *)Q.d_off.p, (uint32_t)nq, k, seed_q.p, seed_i.p, seed_fc.p, d_ns.p);
            launch_1d(k_hit_keep, Q.n_distinct, stream, (const uint32_t *)mult.p, (const uint64_t *)Q.by_number.p, k, 1u, (uint32_t *)nullptr, d_stat.p);
        } else {
            // owner lists as CSR over the distinct words: the kept counts, their scan, the windows sorted by (word, window), the fill
            DevArray<uint32_t> kept(Q.n_distinct);
            occ_off.alloc(Q.n_distinct + 1);
            launch_1d(k_hit_keep, Q.n_distinct, stream, (const uint32_t *)mult.p, (const uint64_t *)Q.by_number.p, k, seed_copies, kept.p, d_stat.p);
            {
                size_t tmp_bytes = 0;
                auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), KeptAt{kept.p, Q.n_distinct});
                SW_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, in, occ_off.p, uint32_t(0), Q.n_distinct + 1, rocprim::plus<uint32_t>(), stream));
                DevArray<unsigned char> tmp(tmp_bytes);
                SW_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, in, occ_off.p, uint32_t(0), Q.n_distinct + 1, rocprim::plus<uint32_t>(), stream));
                SW_HIP(hipStreamSynchronize(stream));
            }
            uint32_t n_owners = 0;   // (<= the valid windows < 2^32)
            SW_HIP(hipMemcpyAsync(&n_owners, occ_off.p + Q.n_distinct, 4, hipMemcpyDeviceToHost, stream));
            SW_HIP(hipStreamSynchronize(stream));
            owners.alloc(n_owners);
            if (n_owners) {
                DevArray<uint64_t> ok_a(Q.n_valid), ok_b(Q.n_valid);
                launch_1d(k_own_keys, Q.n_valid, stream, (const uint32_t *)Q.sidx.p, (const uint32_t *)Q.number.p, ok_a.p);
                uint64_t *kp = ok_a.p, *ap = ok_b.p;
                sort_all_bits(kp, ap, Q.n_valid, stream);
                launch_1d(k_own_fill, Q.n_valid, stream, (const uint64_t *)kp, (const uint32_t *)kept.p, (const uint32_t *)occ_off.p, (const uint64_t *)Q.by_number.p,
                          (const uint32_t *)Q.vpos.p, (const uint8_t *)Q.text.p, (const uint64_t *)Q.d_off.p, (uint32_t)nq, k, owners.p, d_ns.p);
                SW_HIP(hipStreamSynchronize(stream));   // (the sort's buffers are read until here)
            }
        }
        SW_HIP(hipMemcpyAsync(o.n_seeds.data(), d_ns.p, nq * 4, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipMemcpyAsync(seed_stat, d_stat.p, sizeof seed_stat, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
        for (uint32_t s : o.n_seeds) n_seeds_total += s;
    }
    if (n_seeds_total) pack_queries(Q.text.p, offsets, nq, P);
    SW_HIP(hipStreamSynchronize(stream));
    Q.release_temporaries();
    o.n_seeds_total = n_seeds_total;
    SW_HIP(hipEventRecord(e1, stream));
    SW_HIP(hipStreamSynchronize(stream));
    float fms = 0;
    SW_HIP(hipEventElapsedTime(&fms, e0, e1));
    o.ms[0] = fms;

    uint64_t hits = 0, chunks = 0, splits = 0, grows = 0, launches = 0, aligned = 0, striped = 0, cap_keys = 0;
    if (n_seeds_total && n_asm) {
        RunTiles T;
        build_run_tiles(h, k, "best hits", T);
        DevRuns runs(b);
        // the buffer's budget changes speed only; SEQWIN_AMD_HIT_BUFFER_KB (test library) sets it.  Half of it holds keys, half the sort's second buffer
        uint64_t budget = HIT_BUFFER_BYTES;
        if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_HIT_BUFFER_KB")) budget = env_u64(e, budget >> 10) << 10;
        cap_keys = std::min<uint64_t>(std::max<uint64_t>(budget / 16, 1), HIT_MAX_KEYS);
        DevArray<uint64_t> buf_a(cap_keys), buf_b(cap_keys);
        DevArray<uint32_t> d_fail(1), d_np(1);
        DevArray<unsigned long long> d_cursor(1);
        DevRunTiles tiles(T, b.d_packed.p, stream, true);
        HitArgs g{};
        g.t = Q.table();
        g.seed_q = seed_q.p;
        g.seed_i = seed_i.p;
        g.seed_fc = seed_fc.p;
        g.qoff = P.off.p;
        g.cursor = d_cursor.p;
        g.k = k;
        g.band_bits = band_bits;
        g.rec_bits = rec_bits;
        HitSharedArgs gs{};
        gs.t = g.t;
        gs.occ_off = occ_off.p;
        gs.owners = owners.p;
        gs.qoff = P.off.p;
        gs.cursor = d_cursor.p;
        gs.k = k;
        gs.band_bits = band_bits;
        gs.rec_bits = rec_bits;
        const uint32_t blocks_max = launch_blocks("SEQWIN_AMD_HIT_MAX_BLOCKS");   // the probe kernel's; the switch (test library) lowers it
        Event c0, c1, c2, c3;
        uint64_t rows = n_asm;
        for (uint64_t a0 = 0; a0 < n_asm;) {
            const uint64_t a1 = std::min<uint64_t>(n_asm, a0 + rows);
            // probe: the chunk's tiles
            SW_HIP(hipEventRecord(c0, stream));
            SW_HIP(hipMemsetAsync(d_cursor.p, 0, 8, stream));
            g.buf = buf_a.p;
            g.cap = cap_keys;
            g.v = tiles.view(T.asm_tile_off[a0], T.asm_tile_off[a1]);
            if (shared) {
                gs.buf = buf_a.p;
                gs.cap = cap_keys;
                gs.v = g.v;
                launches += launch_tiles(k_hit_probe_shared, gs, blocks_max, stream);
            } else {
                launches += launch_tiles(k_hit_probe, g, blocks_max, stream);
            }
            unsigned long long n_hits = 0;
            SW_HIP(hipMemcpyAsync(&n_hits, d_cursor.p, 8, hipMemcpyDeviceToHost, stream));
            SW_HIP(hipEventRecord(c1, stream));
            SW_HIP(hipStreamSynchronize(stream));
            SW_HIP(hipEventElapsedTime(&fms, c0, c1));
            o.ms[1] += fms;
            if (n_hits > cap_keys) {
                if (a1 - a0 > 1) {   // redone in two halves: the first now, the second is the next chunk
                    rows = (a1 - a0 + 1) / 2;
                    ++splits;
                } else {             // one assembly above the budget: the buffer doubles
                    if (cap_keys >= HIT_MAX_KEYS) raise(SW_ERR_VALUE, "best hits: assembly %llu alone has more than 2^31 hits", (unsigned long long)a0);
                    cap_keys = std::min<uint64_t>(cap_keys * 2, HIT_MAX_KEYS);
                    buf_a.alloc(cap_keys);
                    buf_b.alloc(cap_keys);
                    ++grows;
                }
                continue;
            }
            hits += n_hits;
            o.chunk_hits.push_back(n_hits);
            ++chunks;
            if (n_hits) {
                // sort over the used bits, run heads and lengths
                uint64_t *kp = buf_a.p, *ap = buf_b.p;
                if (n_hits > 1) {
                    SW_HIP(hipMemsetAsync(d_fail.p, 0, 4, stream));
                    sort_keys64(kp, ap, n_hits, 0, key_bits, stream, d_fail.p);
                    uint32_t failed = 0;
                    SW_HIP(hipMemcpyAsync(&failed, d_fail.p, 4, hipMemcpyDeviceToHost, stream));
                    SW_HIP(hipStreamSynchronize(stream));
                    check_sort_failed(failed);
                }
                DevArray<uint8_t> flag(n_hits);
                DevArray<uint32_t> at(n_hits + 1);
                launch_1d(k_scr_heads, n_hits, stream, (const uint64_t *)kp, 0u, flag.p);
                const uint64_t n_runs_k = scan_flags(flag.p, at.p, n_hits, stream);
                DevArray<uint64_t> ukey(n_runs_k);
                DevArray<uint32_t> upos(n_runs_k);
                launch_1d(k_scr_compact, n_hits, stream, (const uint8_t *)flag.p, (const uint32_t *)at.p, (const uint64_t *)kp, ukey.p, upos.p);
                // vote
                const uint64_t c_rows = a1 - a0, cells = nq * c_rows;
                DevArray<unsigned long long> best(cells);
                DevArray<sw_infix_pair> pairs(cells);
                DevArray<uint32_t> out_idx(cells);
                SW_HIP(hipMemsetAsync(best.p, 0, cells * 8, stream));
                SW_HIP(hipMemsetAsync(d_np.p, 0, 4, stream));
                {   // (one range: k_hit_vote reads `end` as the number of runs)
                    const uint64_t blocks = (n_runs_k + SCR_TPB - 1) / SCR_TPB;
                    hipLaunchKernelGGL(k_hit_vote, dim3((unsigned)blocks), dim3(SCR_TPB), 0, stream, (uint64_t)0, n_runs_k, (const uint64_t *)ukey.p,
                                       (const uint32_t *)upos.p, (uint64_t)n_hits, (const uint32_t *)b.d_rec_asm.p, band_bits, rec_bits, (uint32_t)a0, (uint32_t)c_rows,
                                       best.p);
                    SW_HIP(hipGetLastError());
                }
                launch_1d(k_hit_finish, cells, stream, (const unsigned long long *)best.p, (const uint64_t *)ukey.p, (const uint64_t *)P.off.p,
                          (const uint32_t *)runs.t.rec_len, k, band_bits, rec_bits, (uint32_t)a0, (uint32_t)c_rows, n_asm, o.field[0].p, o.field[1].p, o.field[2].p,
                          pairs.p, out_idx.p, d_np.p);
                uint32_t n_pairs = 0;
                SW_HIP(hipMemcpyAsync(&n_pairs, d_np.p, 4, hipMemcpyDeviceToHost, stream));
                SW_HIP(hipEventRecord(c2, stream));
                SW_HIP(hipStreamSynchronize(stream));
                SW_HIP(hipEventElapsedTime(&fms, c1, c2));
                o.ms[2] += fms;
                // Layer A on the chunk's winners
                uint64_t cn[6] = {};
                double dms[1] = {};
                infix_device(runs_of(runs.t), P, pairs.p, out_idx.p, n_pairs, o.field[4].p, o.field[3].p, cn, dms);
                aligned += cn[0];
                striped += cn[2];
                o.ms[3] += dms[0];
                if (align) {
                    uint32_t *const out[4] = {o.afield[0].p, o.afield[1].p, o.afield[2].p, o.afield[3].p};
                    align_device(runs_of(runs.t), P, pairs.p, out_idx.p, n_pairs, o.field[4].p, o.field[3].p, out, nullptr, nullptr, o.align,
                                 pile ? &pile->p->sink : nullptr, pile && pile->w ? &pile->w->sink : nullptr);
                }
                if (local) {
                    uint32_t *lout[LOCAL_FIELDS];
                    for (uint32_t f = 0; f < LOCAL_FIELDS; ++f) lout[f] = o.lfield[f].p;
                    local_device(runs_of(runs.t), P, pairs.p, out_idx.p, n_pairs, *local, lout, o.local);
                }
                if (loci) {
                    // every locus of the chunk's runs: peaks, their list, then Layer A and the traceback as for the winners
                    Event l0, l1;
                    SW_HIP(hipEventRecord(l0, stream));
                    DevArray<uint8_t> peak(n_runs_k);
                    DevArray<uint32_t> peak_at(n_runs_k + 1);
                    launch_1d(k_hit_peaks, n_runs_k, stream, (const uint64_t *)ukey.p, (const uint32_t *)upos.p, n_runs_k, (uint64_t)n_hits, band_bits, min_seeds, peak.p);
                    LociChunk lc;
                    lc.n = scan_flags(peak.p, peak_at.p, n_runs_k, stream);
                    for (int f = 0; f < LF_CHUNK; ++f) lc.f[f].alloc(lc.n);
                    DevArray<sw_infix_pair> lpairs(lc.n);
                    launch_1d(k_hit_loci, n_runs_k, stream, (const uint8_t *)peak.p, (const uint32_t *)peak_at.p, (const uint64_t *)ukey.p, (const uint32_t *)upos.p,
                              n_runs_k, (uint64_t)n_hits, (const uint64_t *)P.off.p, (const uint32_t *)runs.t.rec_len, (const uint32_t *)b.d_rec_asm.p, k, band_bits,
                              rec_bits, lc.ptrs(), lpairs.p);
                    SW_HIP(hipEventRecord(l1, stream));
                    SW_HIP(hipStreamSynchronize(stream));
                    SW_HIP(hipEventElapsedTime(&fms, l0, l1));
                    o.loci.ms[0] += fms;
                    uint64_t lcn[6] = {};
                    double lms[1] = {};
                    infix_device(runs_of(runs.t), P, lpairs.p, nullptr, lc.n, lc.f[LF_DIST].p, lc.f[LF_END].p, lcn, lms);
                    o.loci.ms[1] += lms[0];
                    o.loci.aligned += lcn[0];
                    uint32_t *const lout[4] = {lc.f[LF_START].p, lc.f[LF_NIDENT].p, lc.f[LF_MISMATCH].p, lc.f[LF_GAPS].p};
                    align_device(runs_of(runs.t), P, lpairs.p, nullptr, lc.n, lc.f[LF_DIST].p, lc.f[LF_END].p, lout, nullptr, nullptr, o.loci.align);
                    if (local) {
                        uint32_t *llout[LOCAL_FIELDS];
                        for (uint32_t f = 0; f < LOCAL_FIELDS; ++f) {
                            lc.lf[f].alloc(lc.n);
                            llout[f] = lc.lf[f].p;
                        }
                        local_device(runs_of(runs.t), P, lpairs.p, nullptr, lc.n, *local, llout, o.local);
                    }
                    if (lc.n) loci_chunks.push_back(std::move(lc));
                }
            }
            a0 = a1;
        }
    }
    SW_HIP(hipStreamSynchronize(stream));
    if (pile && pile->w) win_finish(*pile->w, *pile->p, o.align.ms[1]);
    if (pile) pile_finish(*pile->p, o.align.ms[1]);
    if (loci) {
        Event f0, f1;
        SW_HIP(hipEventRecord(f0, stream));
        finish_loci(loci_chunks, nq, n_asm, max_q, stream, o.loci, local != nullptr);
        SW_HIP(hipEventRecord(f1, stream));
        SW_HIP(hipStreamSynchronize(stream));
        SW_HIP(hipEventElapsedTime(&fms, f0, f1));
        o.loci.ms[3] = fms;
        o.loci.ms[2] = o.loci.align.ms[0] + o.loci.align.ms[1];
    }
    const uint64_t cn[10] = {hits, n_seeds_total, chunks, splits, launches, aligned, striped, Q.n_distinct, cap_keys, grows};
    memcpy(o.counters, cn, sizeof cn);
    const uint64_t sc[8] = {seed_copies, seed_stat[SS_WORDS], seed_stat[SS_OCC], seed_stat[SS_DROPPED_WORDS], seed_stat[SS_DROPPED_OCC], seed_stat[SS_PALINDROMES],
                            seed_stat[SS_LONGEST], hits};
    memcpy(o.seed_counters, sc, sizeof sc);
}

}  // namespace

// the checks of a Layer A call, in its order: what a pair says by itself before a handle or a device is touched (arrays_ok: the
// caller's output arrays are there)
void check_infix_pairs(const char *what, const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs, uint64_t n,
                       bool arrays_ok)
{
    check_queries(what, offsets, blob, n_queries);
    if (n && !pairs) raise(SW_ERR_VALUE, "%s: a NULL handle or array", what);
    for (uint64_t i = 0; i < n; ++i)
        if (pairs[i].query >= n_queries || pairs[i].strand > 1 || pairs[i].start > pairs[i].stop)
            raise(SW_ERR_VALUE, "%s: pair %llu (query %u, strand %u, record %u, [%u, %u)) names no query, no strand or no interval", what,
                  (unsigned long long)i, pairs[i].query, pairs[i].strand, pairs[i].record, pairs[i].start, pairs[i].stop);
    if (!b || (n && !arrays_ok)) raise(SW_ERR_VALUE, "%s: a NULL handle or array", what);
    const std::vector<uint32_t> &rec_len = b->host.rec_len;
    for (uint64_t i = 0; i < n; ++i)
        if (pairs[i].record >= rec_len.size() || pairs[i].stop > rec_len[pairs[i].record])
            raise(SW_ERR_VALUE, "%s: pair %llu (record %u, [%u, %u)) does not lie inside one of the batch's %llu records", what, (unsigned long long)i,
                  pairs[i].record, pairs[i].start, pairs[i].stop, (unsigned long long)rec_len.size());
    require_device(b->device, "the batch");
}

namespace {

// min_seeds: nullptr without the loci mode; seed_copies: nullptr for the unique-seed route
void best_hits_entry(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, bool align, const uint64_t *min_seeds,
                     sw_hits **out, const uint64_t *seed_copies = nullptr, const sw_scoring *local = nullptr, PileCall *pile = nullptr, sw_pileup **pile_out = nullptr,
                     sw_windows **win_out = nullptr)
{
    if (k < 1 || k > 32) raise(SW_ERR_VALUE, "best hits: k-mer length must lie in 1..32 (got %llu)", (unsigned long long)k);
    if (seed_copies && (*seed_copies < 1 || *seed_copies > 256))
        raise(SW_ERR_VALUE, "best hits: seed_copies must lie in 1..256 (got %llu)", (unsigned long long)*seed_copies);
    if (min_seeds && !*min_seeds) raise(SW_ERR_VALUE, "best hits: min_seeds must be at least 1 (got 0)");
    if (!batch || !out) raise(SW_ERR_VALUE, "best hits: a NULL handle or array");
    check_queries("best hits", offsets, blob, n_queries);
    if (local)   // a window has at most |query| + 256 bases, and a side of a local alignment stays below 2^16
        for (uint64_t q = 0; q < n_queries; ++q)
            if (offsets[q + 1] - offsets[q] > 65279)
                raise(SW_ERR_VALUE, "best hits: query %llu has %llu bases, above the 65279 the local alignment takes", (unsigned long long)q,
                      (unsigned long long)(offsets[q + 1] - offsets[q]));
    if (pile) {
        if (!pile_out || (pile->lengths && !win_out)) raise(SW_ERR_VALUE, "best hits: a NULL handle or array");
        check_pile_args("best hits", pile->n_groups, pile->max_dist_permille, pile->assembly_group, batch->host.n_assemblies, batch->host.n_assemblies, offsets,
                        n_queries);
    }
    if (batch->host.rec_len.size() && !batch->d_packed.p) raise(SW_ERR_VALUE, "best hits: the batch holds no packed bases (it must be resident)");
    require_device(batch->device, "the batch");
    StreamScope scope(HIT_STREAM);
    std::unique_ptr<sw_hits> o(new sw_hits);
    std::unique_ptr<sw_pileup> po(pile ? new sw_pileup : nullptr);
    std::unique_ptr<sw_windows> wo(pile && pile->lengths ? new sw_windows : nullptr);
    if (pile) pile->p = po.get();
    if (pile) pile->w = wo.get();
    o->device = batch->device;
    batch_best_hits(*batch, offsets, blob, n_queries, (uint32_t)k, align, min_seeds ? *min_seeds : 0, seed_copies ? (uint32_t)*seed_copies : 0u, local, *o, pile);
    *out = o.release();
    if (pile) *pile_out = po.release();
    if (wo) *win_out = wo.release();
}

}  // namespace
}  // namespace sw

using namespace sw;

extern "C" {

int sw_batch_infix_distances(const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs, uint64_t n,
                             uint32_t *dist, uint32_t *end, uint64_t *counters, double *ms)
{
    return guarded([&] {
        check_infix_pairs("infix distances", b, offsets, blob, n_queries, pairs, n, dist && end);
        StreamScope scope(HIT_STREAM);
        DevRuns runs(*b);
        const uint64_t total = n_queries ? offsets[n_queries] : 0;
        DevArray<uint8_t> text(total);
        if (total) SW_HIP(hipMemcpyAsync(text.p, blob, total, hipMemcpyHostToDevice, HIT_STREAM));
        QueryPack P;
        pack_queries(text.p, offsets, n_queries, P);
        DevArray<sw_infix_pair> d_pairs(n);
        DevArray<uint32_t> d_dist(n), d_end(n);
        if (n) SW_HIP(hipMemcpyAsync(d_pairs.p, pairs, n * sizeof(sw_infix_pair), hipMemcpyHostToDevice, HIT_STREAM));
        infix_device(runs_of(runs.t), P, d_pairs.p, nullptr, n, d_dist.p, d_end.p, counters, ms);
        if (n) {
            SW_HIP(hipMemcpy(dist, d_dist.p, n * 4, hipMemcpyDeviceToHost));
            SW_HIP(hipMemcpy(end, d_end.p, n * 4, hipMemcpyDeviceToHost));
        }
    });
}

int sw_batch_best_hits(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, sw_hits **out)
{
    return guarded([&] { best_hits_entry(batch, offsets, blob, n_queries, k, false, nullptr, out); });
}

int sw_batch_best_hits_aligned(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, sw_hits **out)
{
    return guarded([&] { best_hits_entry(batch, offsets, blob, n_queries, k, true, nullptr, out); });
}

int sw_batch_best_hits_loci(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, uint64_t min_seeds, sw_hits **out)
{
    return guarded([&] { best_hits_entry(batch, offsets, blob, n_queries, k, true, &min_seeds, out); });
}

int sw_batch_best_hits_shared(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, uint64_t seed_copies, uint64_t mode,
                              uint64_t min_seeds, sw_hits **out)
{
    return guarded([&] {
        if (mode > 2) raise(SW_ERR_VALUE, "best hits: mode %llu is none of plain, aligned, loci (0..2)", (unsigned long long)mode);
        best_hits_entry(batch, offsets, blob, n_queries, k, mode >= 1, mode == 2 ? &min_seeds : nullptr, out, &seed_copies);
    });
}

int sw_batch_best_hits_local(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, uint64_t seed_copies, uint64_t mode,
                             uint64_t min_seeds, const sw_scoring *scoring, sw_hits **out)
{
    return guarded([&] {
        if (mode > 2) raise(SW_ERR_VALUE, "best hits: mode %llu is none of plain, aligned, loci (0..2)", (unsigned long long)mode);
        check_scoring("best hits", scoring);
        best_hits_entry(batch, offsets, blob, n_queries, k, mode >= 1, mode == 2 ? &min_seeds : nullptr, out, seed_copies ? &seed_copies : nullptr, scoring);
    });
}

int sw_batch_best_hits_pileup(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, uint64_t seed_copies,
                              uint64_t mode, uint64_t min_seeds, const sw_scoring *scoring, const uint8_t *assembly_group, uint64_t n_groups,
                              uint64_t max_dist_permille, sw_hits **out, sw_pileup **pile)
{
    return guarded([&] {
        if (mode > 2) raise(SW_ERR_VALUE, "best hits: mode %llu is none of plain, aligned, loci (0..2)", (unsigned long long)mode);
        if (scoring) check_scoring("best hits", scoring);
        // (the counts of groups and the bound say what they say without the batch; the labels are checked once its assemblies are known)
        check_pile_args("best hits", n_groups, max_dist_permille, nullptr, 0, 0, nullptr, 0);
        PileCall pc{nullptr, assembly_group, n_groups, max_dist_permille};
        best_hits_entry(batch, offsets, blob, n_queries, k, true, mode == 2 ? &min_seeds : nullptr, out, seed_copies ? &seed_copies : nullptr, scoring, &pc, pile);
    });
}

int sw_batch_best_hits_windows(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, uint64_t seed_copies,
                               uint64_t mode, uint64_t min_seeds, const sw_scoring *scoring, const uint8_t *assembly_group, uint64_t n_groups,
                               uint64_t max_dist_permille, const uint32_t *lengths, uint64_t n_lengths, uint64_t max_mismatch, uint64_t three_prime,
                               sw_hits **out, sw_pileup **pile, sw_windows **windows)
{
    return guarded([&] {
        if (mode > 2) raise(SW_ERR_VALUE, "best hits: mode %llu is none of plain, aligned, loci (0..2)", (unsigned long long)mode);
        if (scoring) check_scoring("best hits", scoring);
        check_pile_args("best hits", n_groups, max_dist_permille, nullptr, 0, 0, nullptr, 0);
        check_win_args("best hits", lengths, n_lengths, max_mismatch, three_prime);
        PileCall pc{nullptr, assembly_group, n_groups, max_dist_permille, nullptr, lengths, n_lengths, max_mismatch, three_prime};
        best_hits_entry(batch, offsets, blob, n_queries, k, true, mode == 2 ? &min_seeds : nullptr, out, seed_copies ? &seed_copies : nullptr, scoring, &pc, pile,
                        windows);
    });
}

int sw_hits_seed_stats(const sw_hits *h, uint64_t *counters)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "best hits: a NULL handle");
        if (counters) memcpy(counters, h->seed_counters, sizeof h->seed_counters);
    });
}

static const sw_hits &loci_of(const sw_hits *h)
{
    if (!h) raise(SW_ERR_VALUE, "best hits: a NULL handle");
    if (!h->has_loci) raise(SW_ERR_VALUE, "best hits: these hits were made without the loci (sw_batch_best_hits_loci makes them)");
    return *h;
}

int sw_hits_loci_sizes(const sw_hits *h, uint64_t *n_loci_total, uint64_t *n_dup)
{
    return guarded([&] {
        const HitLoci &l = loci_of(h).loci;
        if (n_loci_total) *n_loci_total = l.n;
        if (n_dup) *n_dup = l.n_dup;
    });
}

int sw_hits_loci(const sw_hits *h, uint64_t *cell_offsets, uint32_t *query, uint32_t *assembly, uint32_t *record, uint32_t *strand, uint32_t *band, uint32_t *seeds,
                 uint32_t *dist, uint32_t *end, uint32_t *a_start, uint32_t *nident, uint32_t *mismatch, uint32_t *gaps, uint32_t *dup)
{
    return guarded([&] {
        const HitLoci &l = loci_of(h).loci;
        require_device(h->device, "the hits");
        if (cell_offsets) SW_HIP(hipMemcpy(cell_offsets, l.cell_off.p, (h->nq * h->n_asm + 1) * 8, hipMemcpyDeviceToHost));
        uint32_t *const out[LOCI_LIST_FIELDS] = {query, assembly, record, strand, band, seeds, dist, end, a_start, nident, mismatch, gaps, dup};
        for (int f = 0; f < LOCI_LIST_FIELDS; ++f)
            if (out[f] && l.n) SW_HIP(hipMemcpy(out[f], l.f[f].p, l.n * 4, hipMemcpyDeviceToHost));
    });
}

int sw_hits_loci_block(const sw_hits *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out)
{
    return guarded([&] {
        const HitLoci &l = loci_of(h).loci;
        if (field > 1) raise(SW_ERR_VALUE, "best hits: field %llu is none of n_loci, sum_nident (0..1)", (unsigned long long)field);
        export_cells("best hits", "queries", h->device, "the hits", field ? l.sum_nident.p : l.n_loci.p, h->nq, h->n_asm, r0, r1, c0, c1, out);
    });
}

int sw_hits_loci_stats(const sw_hits *h, uint64_t *counters, double *ms)
{
    return guarded([&] {
        const HitLoci &l = loci_of(h).loci;
        const uint64_t cn[5] = {l.n, l.n_dup, l.max_per_cell, l.aligned, l.align.counters[1]};
        if (counters) memcpy(counters, cn, sizeof cn);
        if (ms) memcpy(ms, l.ms, sizeof l.ms);
    });
}

int sw_hits_sizes(const sw_hits *h, uint64_t *n_queries, uint64_t *n_assemblies, uint64_t *n_seeds, uint64_t *k)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "best hits: a NULL handle");
        if (n_queries) *n_queries = h->nq;
        if (n_assemblies) *n_assemblies = h->n_asm;
        if (n_seeds) *n_seeds = h->n_seeds_total;
        if (k) *k = h->k;
    });
}

int sw_hits_n_seeds(const sw_hits *h, uint32_t *n_seeds)
{
    return guarded([&] {
        if (!h || (h->nq && !n_seeds)) raise(SW_ERR_VALUE, "best hits: a NULL handle or array");
        if (h->nq) memcpy(n_seeds, h->n_seeds.data(), h->nq * 4);
    });
}

int sw_hits_block(const sw_hits *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "best hits: a NULL handle");
        if (field > 4) raise(SW_ERR_VALUE, "best hits: field %llu is none of seeds, record, strand, end, dist (0..4)", (unsigned long long)field);
        export_cells("best hits", "queries", h->device, "the hits", h->field[field].p, h->nq, h->n_asm, r0, r1, c0, c1, out);
    });
}

int sw_hits_stats(const sw_hits *h, uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "best hits: a NULL handle");
        if (counters) memcpy(counters, h->counters, sizeof h->counters);
        if (ms) memcpy(ms, h->ms, sizeof h->ms);
    });
}

int sw_hits_chunk_hits(const sw_hits *h, uint64_t *hits)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "best hits: a NULL handle");
        if (hits && !h->chunk_hits.empty()) memcpy(hits, h->chunk_hits.data(), h->chunk_hits.size() * 8);
    });
}

void sw_hits_free(sw_hits *h)
{
    delete h;
}

}  // extern "C"
