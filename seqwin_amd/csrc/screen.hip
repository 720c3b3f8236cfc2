// screen.hip -- exact k-mer containment of query sequences in every assembly of a resident batch.
//
// Stands where markers.eval_markers (src/seqwin/markers.py:607-696) BLASTs every representative against every assembly.  It has no
// counterpart in the reference, it is NOT BLAST and it fills none of MarkerMetrics: counts[q, a] = the number of query q's distinct
// canonical k-mers that occur anywhere in assembly a, nothing else (DESIGN.md section 3.2d is the specification;
// tests/tools/screen_host.py restates it).  Keys are the full 2k-bit words: no hash stands for a k-mer, nothing is approximate.
//
//   k_scr_qwords   one thread per byte of the query text: the canonical word of the window that starts there, or "no window"
//   query side     the valid words compacted, a sorted copy made distinct (the library's keys-only radix sort), an open-addressing
//                  table built over the distinct words (k_scr_insert: one atomicCAS per probed slot, no comparison, no waiting),
//                  the distinct words numbered in order of first appearance in the query text (k_scr_first: atomicMin of the
//                  position per word; flag and scan), the table's slots relabelled to those numbers; per query the list of
//                  (bitmap word, mask) pairs that cover its k-mers (sort of query << 32 | number, k_scr_pairs)
//   k_scr_probe    the hot path.  The batch's run / tile / lane walk (kmer_walk.hpp): a tile of 1024 k-mers of one valid run per
//                  wave, 16 consecutive k-mers per lane.  A lane rolls its 16 canonical words, issues their 16 first-slot loads
//                  together, resolves the occupied ones, and sets bit `number` of its assembly's row of a presence bitmap with
//                  atomicOr -- consecutive hits that fall into one bitmap word leave as one atomic
//   k_scr_reduce   counts[q, a] = sum over q's pairs of popcount(bitmap[a][word] & mask): a wave per (query, assembly)
// The bitmap holds a chunk of assemblies (a budget, 1 GiB by default); tiles are ordered by assembly, so a chunk is a tile range.
//
// The k-mer profile (sw_batch_screen_profile; DESIGN.md section 3.2m, tests/tools/kprofile_host.py restates it) reduces the same bitmap
// the other way -- per distinct k-mer and group of assemblies, the rows that hold it -- and reads the result out per text position:
//   k_scr_profile  per chunk, behind k_scr_reduce: bit-sliced vertical counters per lane, a lane per bitmap word, rows in group order
//   k_scr_probe<true>   the probe with one 64-bit atomicAdd per hit into the copies table (only with copies)
//   k_scr_posnum / k_scr_gather   the position -> number map of the query side kept, the tables per number gathered per position
// A screen without a profile launches none of these.
#include "screen_core.hpp"

namespace sw {
namespace {

// ---- probe ----------------------------------------------------------------------------------------------------------------------
struct ProbeArgs {
    RunView v;                       // the tiles of this launch: all of assemblies [asm0, asm0 + rows of the bitmap)
    Table t;                         // slots hold number + 1, keys are in number order
    uint32_t *bitmap;                // [assembly - asm0][words]
    uint32_t asm0;
    uint64_t words;                  // ceil(distinct / 32)
    unsigned long long *stat;        // [0] hits, [1] atomics issued
    uint32_t k;
};

// what the probe with copy counts (the k-mer profile) takes on top
struct ProbeCopyArgs : ProbeArgs {
    const uint8_t *labels;           // [n_asm] the group of every assembly, 255: left out
    unsigned long long *copies;      // [distinct][n_groups]
    uint32_t n_groups;
};

// COPIES = false is the screen's probe as it always was (every addition below sits behind `if constexpr (COPIES)`); true: a hit also
// adds one to copies[number][group of the assembly] (stat[2]: those adds)
template <bool COPIES> __global__ __launch_bounds__(SCR_TPB) void k_scr_probe(std::conditional_t<COPIES, ProbeCopyArgs, ProbeArgs> g)
{
    const uint32_t lane = threadIdx.x % SCR_WAVE;
    uint32_t r, n_mine;
    uint64_t first;
    if (!wave_tile(g.v, lane, r, first, n_mine)) return;   // (the whole wave)
    const uint32_t a = g.v.run_asm[r], k = g.k;
    unsigned long long hits = 0, atomics = 0;
    [[maybe_unused]] uint32_t label = 0xFFu;   // (uniform in the wave: a tile lies in one assembly)
    [[maybe_unused]] unsigned long long adds = 0;
    if constexpr (COPIES) label = g.labels[a];
    KmerRoller R(g.v.packed, k);
    if (n_mine) {
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
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < SCR_L; ++j) {   // the 16 first-slot loads leave together
            home[j] = scr_home(canon[j], g.t.bits);
            slot[j] = j < n_mine ? g.t.slots[home[j]] : 0u;
        }
        uint32_t *row = g.bitmap + (uint64_t)(a - g.asm0) * g.words;
        uint32_t cur_word = SCR_NONE, cur_mask = 0;
#pragma unroll
        for (uint32_t j = 0; j < SCR_L; ++j) {
            if (!slot[j]) continue;
            const uint32_t id = scr_find_from(g.t, canon[j], home[j], slot[j]);
            if (id == SCR_NONE) continue;
            ++hits;
            if constexpr (COPIES) {
                if (label != 0xFFu) {
                    atomicAdd(g.copies + (uint64_t)id * g.n_groups + label, 1ull);
                    ++adds;
                }
            }
            if ((id >> 5) != cur_word) {   // consecutive hits in one bitmap word leave as one atomic
                if (cur_mask) {
                    atomicOr(row + cur_word, cur_mask);
                    ++atomics;
                }
                cur_word = id >> 5;
                cur_mask = 0;
            }
            cur_mask |= 1u << (id & 31);
        }
        if (cur_mask) {
            atomicOr(row + cur_word, cur_mask);
            ++atomics;
        }
    }
    hits = wave_sum(hits);
    atomics = wave_sum(atomics);
    if (lane == 0 && hits) {
        atomicAdd(g.stat, hits);
        atomicAdd(g.stat + 1, atomics);
    }
    if constexpr (COPIES) {
        adds = wave_sum(adds);
        if (lane == 0 && adds) atomicAdd(g.stat + 2, adds);
    }
}

// ---- the k-mer profile: the bitmap reduced the other way ------------------------------------------------
constexpr uint32_t PRF_PLANES = 8;                          // bit-sliced counter planes of a lane: one count per bit of its bitmap word
constexpr uint32_t PRF_FLUSH = (1u << PRF_PLANES) - 1;      // rows the planes take before they are emptied into the lane's 32 counts
constexpr uint32_t PRF_SLICE = 1024;                        // rows of a chunk (in group order) per workgroup; chosen without a measurement
constexpr uint32_t PRF_MAX_GROUPS = 8;

// the planes' 32 counts added to acc, the planes emptied
__device__ __forceinline__ void prf_flush(uint32_t (&plane)[PRF_PLANES], uint32_t (&acc)[32])
{
#pragma unroll
    for (uint32_t b = 0; b < 32; ++b) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t p = 0; p < PRF_PLANES; ++p) c |= ((plane[p] >> b) & 1u) << p;
        acc[b] += c;
    }
#pragma unroll
    for (uint32_t p = 0; p < PRF_PLANES; ++p) plane[p] = 0;
}

// present[number][group] += the rows of the group whose bit `number` is set.  A workgroup takes SCR_TPB consecutive bitmap words -- a
// lane one word of every row, so a wave reads 64 consecutive words of a row -- and a slice of at most PRF_SLICE of the chunk's kept
// rows, which the host has put in group order (order[] / olabel[]: the row in the chunk and its group): the group is uniform and
// changes at most n_groups - 1 times in a slice.  A row's word is added to the lane's planes by a ripple of half adders; the planes
// are emptied into 32 counts every PRF_FLUSH rows, the counts leave once per (word tile, slice, group), one atomicAdd per non-zero count.
__global__ __launch_bounds__(SCR_TPB) void k_scr_profile(const uint32_t *__restrict__ bitmap, uint64_t words, uint64_t n_distinct,
                                                         const uint32_t *__restrict__ order, const uint8_t *__restrict__ olabel, uint32_t n_kept,
                                                         uint32_t n_groups, uint64_t block0, uint32_t slices, uint32_t *__restrict__ present)
{
    const uint64_t blk = block0 + blockIdx.x;
    const uint64_t w = (blk / slices) * SCR_TPB + threadIdx.x;
    const uint32_t i0 = (uint32_t)(blk % slices) * PRF_SLICE, i1 = i0 + PRF_SLICE < n_kept ? i0 + PRF_SLICE : n_kept;
    if (i0 >= i1) return;   // (the whole workgroup; the host launches no such slice)
    const bool mine = w < words;
    uint32_t plane[PRF_PLANES], acc[32];
#pragma unroll
    for (uint32_t p = 0; p < PRF_PLANES; ++p) plane[p] = 0;
#pragma unroll
    for (uint32_t b = 0; b < 32; ++b) acc[b] = 0;
    uint32_t in_planes = 0, group = olabel[i0];
    for (uint32_t i = i0; i <= i1; ++i) {   // (i == i1: the last group leaves)
        const uint32_t gi = i < i1 ? olabel[i] : 0xFFFFFFFFu;
        if (gi != group) {
            prf_flush(plane, acc);
            in_planes = 0;
            if (mine) {
#pragma unroll
                for (uint32_t b = 0; b < 32; ++b) {
                    const uint64_t number = w * 32 + b;
                    if (acc[b] && number < n_distinct) atomicAdd(present + number * n_groups + group, acc[b]);
                    acc[b] = 0;
                }
            }
            group = gi;
            if (i == i1) break;
        } else if (in_planes == PRF_FLUSH) {
            prf_flush(plane, acc);
            in_planes = 0;
        }
        uint32_t carry = mine ? bitmap[(uint64_t)order[i] * words + w] : 0u;
#pragma unroll
        for (uint32_t p = 0; p < PRF_PLANES; ++p) {
            const uint32_t t = plane[p] & carry;
            plane[p] ^= carry;
            carry = t;
        }
        ++in_planes;
    }
}

// pnum[text position] = the number of the distinct word whose window starts there (pnum is SCR_NONE everywhere else)
__global__ __launch_bounds__(SCR_TPB) void k_scr_posnum(uint64_t base, uint64_t end, const uint32_t *__restrict__ vpos, const uint32_t *__restrict__ sidx,
                                                        const uint32_t *__restrict__ number, uint32_t *__restrict__ pnum)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j < end) pnum[vpos[j]] = number[sidx[j]];
}

// the per-number tables read out per text position; a position where no window starts gets all ones.  copies / out_copies may be null
__global__ __launch_bounds__(SCR_TPB) void k_scr_gather(uint64_t base, uint64_t end, const uint32_t *__restrict__ pnum, uint32_t n_groups,
                                                        const uint32_t *__restrict__ present, const unsigned long long *__restrict__ copies,
                                                        uint32_t *__restrict__ out_present, unsigned long long *__restrict__ out_copies)
{
    const uint64_t p = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (p >= end) return;
    const uint32_t num = pnum[p];
    for (uint32_t g = 0; g < n_groups; ++g) {
        out_present[p * n_groups + g] = num == SCR_NONE ? 0xFFFFFFFFu : present[(uint64_t)num * n_groups + g];
        if (out_copies) out_copies[p * n_groups + g] = num == SCR_NONE ? ~0ull : copies[(uint64_t)num * n_groups + g];
    }
}

// counts[q][asm0 + r] for queries [q0, q0 + gridDim.x / row_tiles) and the bitmap's rows: a wave per (query, row), the lanes over
// the query's pairs
__global__ __launch_bounds__(SCR_TPB) void k_scr_reduce(const uint32_t *__restrict__ bitmap, uint64_t words, uint32_t asm0, uint32_t rows, uint64_t n_asm,
                                                        uint32_t q0, uint32_t row_tiles, const uint64_t *__restrict__ pair_off,
                                                        const uint32_t *__restrict__ pword, const uint32_t *__restrict__ pmask, uint32_t *__restrict__ counts)
{
    const uint32_t wave = threadIdx.x / SCR_WAVE, lane = threadIdx.x % SCR_WAVE;
    const uint32_t q = q0 + blockIdx.x / row_tiles, rt = blockIdx.x % row_tiles;
    const uint64_t p0 = pair_off[q], p1 = pair_off[q + 1];
    const uint32_t r_end = (rt + 1) * SCR_RED_ROWS < rows ? (rt + 1) * SCR_RED_ROWS : rows;
    for (uint32_t r = rt * SCR_RED_ROWS + wave; r < r_end; r += SCR_WPB) {   // (uniform in the wave)
        const uint32_t *row = bitmap + (uint64_t)r * words;
        unsigned long long s = 0;
        for (uint64_t i = p0 + lane; i < p1; i += SCR_WAVE) s += (unsigned long long)__popc(row[pword[i]] & pmask[i]);
        s = wave_sum(s);
        if (lane == 0) counts[(uint64_t)q * n_asm + asm0 + r] = (uint32_t)s;
    }
}

}  // namespace
}  // namespace sw

struct sw_screen {
    int device = 0;
    uint64_t nq = 0, n_asm = 0, n_distinct = 0, k = 0;
    std::vector<uint32_t> n_kmers;         // [nq] distinct canonical k-mers of every query
    sw::DevArray<uint32_t> counts;         // [nq][n_asm]
    uint64_t counters[10] = {};            // sw_screen_stats
    double ms[3] = {};                     // table build, probe, reduce
    std::vector<double> chunk_probe_ms, chunk_reduce_ms;
    // the k-mer profile of sw_batch_screen_profile; none of it exists in a plain screen
    bool profiled = false, has_copies = false;
    uint64_t prof_rows = 0, prof_groups = 0;             // rows: the bytes of the query text
    sw::DevArray<uint32_t> present;                      // [prof_rows][prof_groups]
    sw::DevArray<unsigned long long> copies;             // [prof_rows][prof_groups], with has_copies
    std::vector<uint32_t> group_sizes;                   // [prof_groups]
    uint64_t prof_counters[2] = {};                      // table bytes, copy adds issued
    double prof_ms[2] = {};                              // k_scr_profile, k_scr_gather
};

namespace sw {
namespace {

struct ProfileCall {
    const uint8_t *labels;   // [n_asm]
    uint32_t n_groups;
    bool copies;
};

// pc: null for the plain screen, which then launches what it always launched
void batch_screen(const sw_batch &b, const uint64_t *offsets, const char *blob, uint64_t nq, uint32_t k, hipStream_t stream, sw_screen &o,
                  const ProfileCall *pc = nullptr)
{
    const HostBatch &h = b.host;
    const uint64_t n_asm = h.n_assemblies, text_bytes = nq ? offsets[nq] : 0;
    if (n_asm > SCR_MAX_BLOCKS) raise(SW_ERR_VALUE, "screen: %llu assemblies exceed one launch (%u)", (unsigned long long)n_asm, SCR_MAX_BLOCKS);
    if (h.rec_len.size() && !b.d_packed.p) raise(SW_ERR_VALUE, "screen: the batch holds no packed bases (it must be resident)");
    o.nq = nq;
    o.n_asm = n_asm;
    o.k = k;
    o.n_kmers.assign(nq, 0);
    o.counts.alloc(nq * n_asm);
    if (nq * n_asm) SW_HIP(hipMemsetAsync(o.counts.p, 0, nq * n_asm * 4, stream));
    auto up = [&](void *dst, const void *src, size_t bytes) {
        if (bytes) SW_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    };
    Event e0, e1;
    SW_HIP(hipEventRecord(e0, stream));

    // ---- query side: distinct canonical words, the table, numbers by first appearance (screen_core.hpp), (word, mask) pairs per query ----
    QuerySide Q;
    build_query_side(offsets, blob, nq, k, stream, Q);
    const uint64_t n_valid = Q.n_valid, n_distinct = Q.n_distinct, cap = Q.cap;
    uint64_t n_pairs = 0;
    const uint32_t bits = Q.bits, chain = Q.chain;
    DevArray<uint32_t> pword, pmask;
    DevArray<uint64_t> pair_off(nq + 1);
    std::vector<uint64_t> pair_off_host(nq + 1, 0);
    if (n_valid) {
        // pairs: (query << 32 | number) ascending; a run of equal (query, number >> 5) is one pair
        launch_1d(k_scr_qkeys, n_valid, stream, (const uint32_t *)Q.vpos.p, (const uint32_t *)Q.sidx.p, (const uint32_t *)Q.number.p, (const uint64_t *)Q.d_off.p,
                  (uint32_t)nq, Q.s_a.p);
        uint64_t *kp = Q.s_a.p, *ap = Q.s_b.p;
        sort_all_bits(kp, ap, n_valid, stream);
        launch_1d(k_scr_heads, n_valid, stream, (const uint64_t *)kp, 5u, Q.flag.p);
        n_pairs = scan_flags(Q.flag.p, Q.at.p, n_valid, stream);
        pword.alloc(n_pairs);
        pmask.alloc(n_pairs);
        DevArray<uint32_t> d_np(nq), d_nk(nq);
        SW_HIP(hipMemsetAsync(pmask.p, 0, n_pairs * 4, stream));
        SW_HIP(hipMemsetAsync(d_np.p, 0, nq * 4, stream));
        SW_HIP(hipMemsetAsync(d_nk.p, 0, nq * 4, stream));
        launch_1d(k_scr_pairs, n_valid, stream, (const uint64_t *)kp, (const uint8_t *)Q.flag.p, (const uint32_t *)Q.at.p, pword.p, pmask.p, d_np.p, d_nk.p);
        std::vector<uint32_t> np(nq);
        SW_HIP(hipMemcpyAsync(np.data(), d_np.p, nq * 4, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipMemcpyAsync(o.n_kmers.data(), d_nk.p, nq * 4, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
        for (uint64_t q = 0; q < nq; ++q) pair_off_host[q + 1] = pair_off_host[q] + np[q];
        if (pair_off_host[nq] != n_pairs) raise(SW_ERR_RUNTIME, "internal error: the queries' pair lists do not add up");
    }
    // the profile keeps the position -> number map of the query side, and the tables per number the chunks add to
    const uint32_t ng = pc ? pc->n_groups : 0;
    DevArray<uint32_t> pnum, dpresent;
    DevArray<unsigned long long> dcopies;
    if (pc) {
        o.profiled = true;
        o.has_copies = pc->copies;
        o.prof_rows = text_bytes;
        o.prof_groups = ng;
        o.group_sizes.assign(ng, 0);
        for (uint64_t a = 0; a < n_asm; ++a)
            if (pc->labels[a] != 0xFF) ++o.group_sizes[pc->labels[a]];
        pnum.alloc(text_bytes);
        dpresent.alloc(n_distinct * ng);
        if (text_bytes) SW_HIP(hipMemsetAsync(pnum.p, 0xFF, text_bytes * 4, stream));
        if (n_distinct) SW_HIP(hipMemsetAsync(dpresent.p, 0, n_distinct * ng * 4, stream));
        if (pc->copies) {
            dcopies.alloc(n_distinct * ng);
            if (n_distinct) SW_HIP(hipMemsetAsync(dcopies.p, 0, n_distinct * ng * 8, stream));
        }
        if (n_valid)
            launch_1d(k_scr_posnum, n_valid, stream, (const uint32_t *)Q.vpos.p, (const uint32_t *)Q.sidx.p, (const uint32_t *)Q.number.p, pnum.p);
    }
    Q.release_temporaries();
    DevArray<uint32_t> &slots = Q.slots;
    DevArray<uint64_t> &by_number = Q.by_number;
    up(pair_off.p, pair_off_host.data(), (nq + 1) * 8);
    o.n_distinct = n_distinct;
    SW_HIP(hipEventRecord(e1, stream));

    // ---- the valid runs of length >= k, once per call (kmer_walk.hpp) ----
    RunTiles T;
    build_run_tiles(h, k, "screen", T);
    const std::vector<uint64_t> &asm_kmers = T.asm_kmers;
    const std::vector<uint32_t> &asm_tile_off = T.asm_tile_off;

    // ---- probe and reduce, a chunk of assemblies at a time ----
    uint64_t probed = 0, launches = 0, chunks = 0;
    unsigned long long stat[2] = {};
    std::vector<std::unique_ptr<Event>> ev, pev;
    if (n_distinct && n_asm && nq) {
        const uint64_t words = (n_distinct + 31) / 32;
        // the bitmap's budget changes speed only; 1 GiB has no measurement behind it.  SEQWIN_AMD_SCR_BITMAP_KB (test library) sets it
        uint64_t budget = SCR_BITMAP_BYTES;
        if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_SCR_BITMAP_KB")) budget = env_u64(e, budget >> 10) << 10;
        const uint64_t rows_max = std::min<uint64_t>(std::max<uint64_t>(budget / (words * 4), 1), n_asm);
        DevArray<uint32_t> bitmap(rows_max * words);
        DevRunTiles runs(T, b.d_packed.p, stream);
        DevArray<unsigned long long> d_stat(3);
        SW_HIP(hipMemsetAsync(d_stat.p, 0, 24, stream));
        SW_HIP(hipMemsetAsync(bitmap.p, 0, rows_max * words * 4, stream));
        ProbeArgs g{};
        g.t = Table{slots.p, by_number.p, cap, bits};
        g.bitmap = bitmap.p;
        g.words = words;
        g.stat = d_stat.p;
        g.k = k;
        const uint32_t blocks_max = launch_blocks(SCR_BLOCKS_ENV);
        const uint32_t q_step = (uint32_t)std::max<uint64_t>(blocks_max / ((rows_max + SCR_RED_ROWS - 1) / SCR_RED_ROWS), 1);
        // the profile's rows: every chunk's kept rows in group order (a stable sort: a counting pass per chunk), at the chunk's place
        ProbeCopyArgs gc{};
        std::vector<uint32_t> kept_of_chunk;
        DevArray<uint32_t> d_order;
        DevArray<uint8_t> d_olabel, d_labels;
        if (pc) {
            std::vector<uint32_t> order(n_asm);
            std::vector<uint8_t> olabel(n_asm, 0xFF);
            for (uint64_t a0 = 0; a0 < n_asm; a0 += rows_max) {
                const uint64_t a1 = std::min<uint64_t>(n_asm, a0 + rows_max);
                uint64_t at = a0;
                for (uint32_t grp = 0; grp < ng; ++grp)
                    for (uint64_t a = a0; a < a1; ++a)
                        if (pc->labels[a] == grp) {
                            order[at] = (uint32_t)(a - a0);
                            olabel[at++] = (uint8_t)grp;
                        }
                kept_of_chunk.push_back((uint32_t)(at - a0));
            }
            d_order.alloc(n_asm);
            d_olabel.alloc(n_asm);
            up(d_order.p, order.data(), n_asm * 4);
            up(d_olabel.p, olabel.data(), n_asm);
            if (pc->copies) {
                d_labels.alloc(n_asm);
                up(d_labels.p, pc->labels, n_asm);
            }
            SW_HIP(hipStreamSynchronize(stream));   // (order and olabel leave this block)
        }
        for (uint64_t a0 = 0; a0 < n_asm; a0 += rows_max, ++chunks) {
            const uint64_t a1 = std::min<uint64_t>(n_asm, a0 + rows_max), rows = a1 - a0;
            for (int i = 0; i < 3; ++i) ev.emplace_back(new Event);
            SW_HIP(hipEventRecord(*ev[3 * chunks], stream));
            g.asm0 = (uint32_t)a0;
            g.v = runs.view(asm_tile_off[a0], asm_tile_off[a1]);
            if (pc && pc->copies) {
                static_cast<ProbeArgs &>(gc) = g;
                gc.labels = d_labels.p;
                gc.copies = dcopies.p;
                gc.n_groups = ng;
                launches += launch_tiles(k_scr_probe<true>, gc, blocks_max, stream);
            } else {
                launches += launch_tiles(k_scr_probe<false>, g, blocks_max, stream);
            }
            probed += asm_kmers[a1] - asm_kmers[a0];
            SW_HIP(hipEventRecord(*ev[3 * chunks + 1], stream));
            const uint32_t row_tiles = (uint32_t)((rows + SCR_RED_ROWS - 1) / SCR_RED_ROWS);
            for (uint64_t q0 = 0; q0 < nq; q0 += q_step) {
                const uint64_t qn = std::min<uint64_t>(q_step, nq - q0);
                hipLaunchKernelGGL(k_scr_reduce, dim3((unsigned)(qn * row_tiles)), dim3(SCR_TPB), 0, stream, (const uint32_t *)bitmap.p, words, (uint32_t)a0,
                                   (uint32_t)rows, n_asm, (uint32_t)q0, row_tiles, (const uint64_t *)pair_off.p, (const uint32_t *)pword.p,
                                   (const uint32_t *)pmask.p, o.counts.p);
                SW_HIP(hipGetLastError());
            }
            if (pc) {   // the same bitmap reduced the other way, before it is cleared
                for (int i = 0; i < 2; ++i) pev.emplace_back(new Event);
                SW_HIP(hipEventRecord(*pev[2 * chunks], stream));
                const uint32_t kept = kept_of_chunk[chunks];
                const uint32_t slices = (kept + PRF_SLICE - 1) / PRF_SLICE;
                const uint64_t total = (words + SCR_TPB - 1) / SCR_TPB * slices;
                for (uint64_t b0 = 0; b0 < total; b0 += blocks_max) {
                    hipLaunchKernelGGL(k_scr_profile, dim3((unsigned)std::min<uint64_t>(blocks_max, total - b0)), dim3(SCR_TPB), 0, stream,
                                       (const uint32_t *)bitmap.p, words, n_distinct, (const uint32_t *)d_order.p + a0, (const uint8_t *)d_olabel.p + a0, kept, ng,
                                       b0, slices, dpresent.p);
                    SW_HIP(hipGetLastError());
                }
                SW_HIP(hipEventRecord(*pev[2 * chunks + 1], stream));
            }
            if (a1 < n_asm) SW_HIP(hipMemsetAsync(bitmap.p, 0, rows * words * 4, stream));   // (cleared for the next chunk)
            SW_HIP(hipEventRecord(*ev[3 * chunks + 2], stream));
        }
        SW_HIP(hipMemcpyAsync(stat, d_stat.p, 16, hipMemcpyDeviceToHost, stream));
        if (pc) SW_HIP(hipMemcpyAsync(&o.prof_counters[1], d_stat.p + 2, 8, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));   // (the temporaries go back to the pool behind the kernels)
    }
    Event g0, g1;
    if (pc) {   // the tables per number read out per text position
        o.present.alloc(text_bytes * ng);
        if (pc->copies) o.copies.alloc(text_bytes * ng);
        SW_HIP(hipEventRecord(g0, stream));
        if (text_bytes)
            launch_1d(k_scr_gather, text_bytes, stream, (const uint32_t *)pnum.p, ng, (const uint32_t *)dpresent.p, (const unsigned long long *)dcopies.p,
                      o.present.p, o.copies.p);
        SW_HIP(hipEventRecord(g1, stream));
        o.prof_counters[0] = pnum.bytes() + dpresent.bytes() + dcopies.bytes() + o.present.bytes() + o.copies.bytes();
    }
    SW_HIP(hipStreamSynchronize(stream));
    float ms = 0;
    SW_HIP(hipEventElapsedTime(&ms, e0, e1));
    o.ms[0] = ms;
    if (pc) {
        SW_HIP(hipEventElapsedTime(&ms, g0, g1));
        o.prof_ms[1] = ms;
    }
    for (uint64_t c = 0; c < chunks; ++c) {
        SW_HIP(hipEventElapsedTime(&ms, *ev[3 * c], *ev[3 * c + 1]));
        o.chunk_probe_ms.push_back(ms);
        o.ms[1] += ms;
        SW_HIP(hipEventElapsedTime(&ms, *ev[3 * c + 1], *ev[3 * c + 2]));
        if (pc) {   // (the profile kernel ran between the two events: its time is its own)
            float pms = 0;
            SW_HIP(hipEventElapsedTime(&pms, *pev[2 * c], *pev[2 * c + 1]));
            o.prof_ms[0] += pms;
            ms = ms > pms ? ms - pms : 0;
        }
        o.chunk_reduce_ms.push_back(ms);
        o.ms[2] += ms;
    }
    const uint64_t cn[10] = {text_bytes, n_valid, n_distinct, cap, chain, probed, stat[0], stat[1], chunks, launches};
    memcpy(o.counters, cn, sizeof cn);
}

}  // namespace
}  // namespace sw

using namespace sw;

// the screen behind a profile getter; a screen made without a profile answers none of them
static const sw_screen &profiled(const sw_screen *h)
{
    if (!h) raise(SW_ERR_VALUE, "screen: a NULL handle");
    if (!h->profiled) raise(SW_ERR_VALUE, "screen: this screen was made without a profile (sw_batch_screen_profile makes one)");
    return *h;
}

extern "C" {

int sw_batch_screen(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, void *stream, sw_screen **out)
{
    return guarded([&] {
        if (k < 1 || k > 32) raise(SW_ERR_VALUE, "screen: k-mer length must lie in 1..32 (got %llu)", (unsigned long long)k);
        if (!batch || !out) raise(SW_ERR_VALUE, "screen: a NULL handle or array");
        check_queries("screen", offsets, blob, n_queries);
        require_device(batch->device, "the batch");
        StreamScope scope((hipStream_t)stream);
        std::unique_ptr<sw_screen> o(new sw_screen);
        o->device = batch->device;
        batch_screen(*batch, offsets, blob, n_queries, (uint32_t)k, (hipStream_t)stream, *o);
        *out = o.release();
    });
}

int sw_batch_screen_profile(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, const uint8_t *labels,
                            uint64_t n_groups, int copies, void *stream, sw_screen **out)
{
    return guarded([&] {
        if (k < 1 || k > 32) raise(SW_ERR_VALUE, "screen: k-mer length must lie in 1..32 (got %llu)", (unsigned long long)k);
        if (!batch || !out) raise(SW_ERR_VALUE, "screen: a NULL handle or array");
        check_queries("screen", offsets, blob, n_queries);
        if (n_groups < 1 || n_groups > PRF_MAX_GROUPS)
            raise(SW_ERR_VALUE, "screen: the profile takes 1..%u groups (got %llu)", PRF_MAX_GROUPS, (unsigned long long)n_groups);
        const uint64_t n_asm = batch->host.n_assemblies;
        if (n_asm && !labels) raise(SW_ERR_VALUE, "screen: a NULL handle or array");
        for (uint64_t a = 0; a < n_asm; ++a)
            if (labels[a] != 0xFF && labels[a] >= n_groups)
                raise(SW_ERR_VALUE, "screen: the group label %u of assembly %llu is neither below the %llu groups nor 255", (unsigned)labels[a],
                      (unsigned long long)a, (unsigned long long)n_groups);
        require_device(batch->device, "the batch");
        StreamScope scope((hipStream_t)stream);
        std::unique_ptr<sw_screen> o(new sw_screen);
        o->device = batch->device;
        const ProfileCall pc{labels, (uint32_t)n_groups, copies != 0};
        batch_screen(*batch, offsets, blob, n_queries, (uint32_t)k, (hipStream_t)stream, *o, &pc);
        *out = o.release();
    });
}

int sw_screen_profile_sizes(const sw_screen *h, uint64_t *rows, uint64_t *n_groups, uint64_t *has_copies)
{
    return guarded([&] {
        const sw_screen &s = profiled(h);
        if (rows) *rows = s.prof_rows;
        if (n_groups) *n_groups = s.prof_groups;
        if (has_copies) *has_copies = s.has_copies ? 1 : 0;
    });
}

int sw_screen_profile_export(const sw_screen *h, uint32_t *present, uint64_t *copies, uint32_t *group_sizes)
{
    return guarded([&] {
        const sw_screen &s = profiled(h);
        if (copies && !s.has_copies) raise(SW_ERR_VALUE, "screen: this profile was made without copy counts");
        if (group_sizes) memcpy(group_sizes, s.group_sizes.data(), s.prof_groups * 4);
        const uint64_t n = s.prof_rows * s.prof_groups;
        if (!n || (!present && !copies)) return;
        require_device(s.device, "the screen");
        if (present) SW_HIP(hipMemcpy(present, s.present.p, n * 4, hipMemcpyDeviceToHost));
        if (copies) SW_HIP(hipMemcpy(copies, s.copies.p, n * 8, hipMemcpyDeviceToHost));
    });
}

int sw_screen_profile_stats(const sw_screen *h, uint64_t *counters, double *ms)
{
    return guarded([&] {
        const sw_screen &s = profiled(h);
        if (counters) memcpy(counters, s.prof_counters, sizeof s.prof_counters);
        if (ms) memcpy(ms, s.prof_ms, sizeof s.prof_ms);
    });
}

int sw_screen_sizes(const sw_screen *h, uint64_t *n_queries, uint64_t *n_assemblies, uint64_t *n_distinct, uint64_t *k)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "screen: a NULL handle");
        if (n_queries) *n_queries = h->nq;
        if (n_assemblies) *n_assemblies = h->n_asm;
        if (n_distinct) *n_distinct = h->n_distinct;
        if (k) *k = h->k;
    });
}

int sw_screen_n_kmers(const sw_screen *h, uint32_t *n_kmers)
{
    return guarded([&] {
        if (!h || (h->nq && !n_kmers)) raise(SW_ERR_VALUE, "screen: a NULL handle or array");
        if (h->nq) memcpy(n_kmers, h->n_kmers.data(), h->nq * 4);
    });
}

int sw_screen_counts(const sw_screen *h, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *counts)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "screen: a NULL handle");
        export_cells("screen", "queries", h->device, "the screen", h->counts.p, h->nq, h->n_asm, r0, r1, c0, c1, counts);
    });
}

int sw_screen_stats(const sw_screen *h, uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "screen: a NULL handle");
        if (counters) memcpy(counters, h->counters, sizeof h->counters);
        if (ms) memcpy(ms, h->ms, sizeof h->ms);
    });
}

int sw_screen_chunk_ms(const sw_screen *h, double *probe_ms, double *reduce_ms)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "screen: a NULL handle");
        const size_t n = h->chunk_probe_ms.size();
        if (probe_ms && n) memcpy(probe_ms, h->chunk_probe_ms.data(), n * 8);
        if (reduce_ms && n) memcpy(reduce_ms, h->chunk_reduce_ms.data(), n * 8);
    });
}

void sw_screen_free(sw_screen *h)
{
    delete h;
}

}  // extern "C"
