// hits_core.hpp -- what hits.hip (seed vote + infix distance) and align.hip (the traceback behind that distance) share: the packed
// queries, the result object, and the host entry points each file offers the other.  Host functions link across the two files;
// device functions do not, so the one both need (plane32) lives here.
#pragma once
#include <vector>

#include "screen_core.hpp"
#include "seqs_core.hpp"

namespace sw {

// Strand s of the query text: base x of query q lies at index off[q] + x of stream s; stream 1 holds the reverse complements.
// codes: 16 bases per word as the batch packs them; valid: a bit per base.
struct QueryPack {
    DevArray<uint32_t> codes[2], valid[2];
    DevArray<uint64_t> off;   // [nq + 1]
    uint64_t nq = 0;
};

// counters[8] = { pairs traced, rounds, pairs on the striped route, pairs with a scratch of their own, scratch bytes at peak, ops
// written, largest scratch of one pair in bytes, launches of the store kernels }; ms[2] = { store pass, walk }
struct AlignStats {
    uint64_t counters[8] = {};
    double ms[2] = {};
};

// The local alignment (local.hip): score, qstart, qend, sstart, send, nident, mismatch, gapopen, gaps.
// counters[6] = { pairs, sum of m * n, pairs in more than one stripe, pairs with an HBM carry row, launches, rows of a group pass }
constexpr uint32_t LOCAL_FIELDS = 9;
struct LocalStats {
    uint64_t counters[6] = {};
    double ms[1] = {};
};

// Every seeded locus of a call made in loci mode, in the list's final order (query, record, strand, band).
// counters-to-be: n, n_dup, max_per_cell, aligned; ms[4] = { peaks + compact, distances, traceback, final ordering + reduction }
constexpr int LOCI_LIST_FIELDS = 13;   // query, assembly, record, strand, band, seeds, dist, end, start, nident, mismatch, gaps, dup
struct HitLoci {
    uint64_t n = 0, n_dup = 0, max_per_cell = 0, aligned = 0, min_seeds = 0;
    DevArray<uint32_t> f[LOCI_LIST_FIELDS];   // [n] each
    DevArray<uint64_t> cell_off;              // [nq * n_asm + 1]
    DevArray<uint32_t> n_loci, sum_nident;    // [nq][n_asm]
    AlignStats align;                         // the loci's traceback (the winners' own stays in sw_hits::align)
    DevArray<uint32_t> lf[LOCAL_FIELDS];               // [n] each: the local alignment's nine figures (made with a scoring system only)
    double ms[4] = {};
};

// The pileup's sink of a traceback (align.hip): where the pile walk adds what it sees.  The label of the pair
// with out index x is group[x] (group_mod == 0: a label per pair) or group[x % group_mod] (a label per assembly of a hits matrix).
constexpr uint32_t PILE_CLASSES = 8;   // A, C, G, T, N, DEL, INS, INS_BASES
constexpr uint8_t PILE_LEAVE_OUT = 0xFF;
enum { PS_PILED, PS_FILTERED, PS_LEFT_OUT, PS_ADDS, PS_N };
struct PileSink {
    uint32_t *table;             // [total query bases][n_groups][PILE_CLASSES]
    uint32_t *depth;             // [nq][n_groups]
    const uint8_t *group;
    uint64_t group_mod;
    uint32_t n_groups, max_dist_permille;
    unsigned long long *stat;    // [PS_N]
};

// The oligo windows' sink of a traceback (align.hip): where the window walk adds the class of every imperfect
// window of a piled pair.  It always travels with a PileSink, whose labels, groups and bound decide which pairs count.
constexpr uint32_t WIN_CLASSES = 8;       // MM0, MM1, MM2, MM3, MM4P, GAPPED, FWD_OK, REV_OK
constexpr uint32_t WIN_MAX_LENGTHS = 8;
enum { WS_WINDOWS, WS_ADDS, WS_N };
struct WinSink {
    uint32_t *table;             // [total query bases][n_lengths][n_groups][WIN_CLASSES]
    uint32_t len[WIN_MAX_LENGTHS];
    uint32_t n_lengths, max_mismatch, three_prime;
    unsigned long long *stat;    // [WS_N]
};

// RunTable (seqs_core.hpp) has internal linkage like every type of that header; this is the same table as the two files hand it to
// each other (runs_of / table_of below)
struct Runs {
    const uint32_t *packed;
    const uint64_t *rec_base;
    const uint32_t *rec_len, *rec_run_off, *run_pos, *run_len;
    uint64_t n_records;
};

// hits.hip
void pack_queries(const uint8_t *d_text, const uint64_t *offsets, uint64_t nq, QueryPack &P);
void infix_device(const Runs &t, const QueryPack &P, const sw_infix_pair *d_pairs, const uint32_t *d_out_idx, uint64_t n, uint32_t *d_dist, uint32_t *d_end,
                  uint64_t *counters, double *ms_out);
void check_infix_pairs(const char *what, const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs, uint64_t n,
                       bool arrays_ok);

// align.hip: the canonical traceback of n valid pairs (device list) whose Layer A results lie at d_dist / d_end [out index of the
// pair].  out[4] = a_start, nident, mismatch, gaps at the same index.  d_ops != nullptr: pair i's script is written so that it ends
// at d_ops[d_ops_end[i]] (exclusive), the slot in front of it holding |query| + dist bytes.  st is added to.
// pile != nullptr: the pile walk stands in for the plain walk -- the same four figures, and every piled pair's columns added to the
// sink; nullptr: not one kernel or argument differs from a call made before the pileup existed.
// win != nullptr (it needs pile): the window walk stands in for the pile walk -- the same figures and the same adds to pile, and every
// imperfect window of a piled pair added to win; nullptr: not one kernel or argument differs from a call made before the windows existed.
void align_device(const Runs &t, const QueryPack &P, const sw_infix_pair *d_pairs, const uint32_t *d_out_idx, uint64_t n, const uint32_t *d_dist,
                  const uint32_t *d_end, uint32_t *const out[4], uint8_t *d_ops, const uint64_t *d_ops_end, AlignStats &st,
                  const PileSink *pile = nullptr, const WinSink *win = nullptr);
// align.hip: the pileup's argument checks (before a device is touched), its zeroed tables, the sink that adds to them, its counters
void check_pile_args(const char *what, uint64_t n_groups, uint64_t max_dist_permille, const uint8_t *labels, uint64_t n_labels, uint64_t n_piles,
                     const uint64_t *offsets, uint64_t nq);
void pile_begin(sw_pileup &p, int device, const uint64_t *offsets, uint64_t nq, uint64_t n_groups, uint64_t max_dist_permille, const uint8_t *labels,
                uint64_t n_labels, uint64_t group_mod);
void pile_finish(sw_pileup &p, double walk_ms);
// align.hip: the oligo windows' argument checks (before a device is touched), their zeroed table and sink, and the finishing pass
// that fills MM0 from the pileup's depths (after the last walk, before pile_finish)
void check_win_args(const char *what, const uint32_t *lengths, uint64_t n_lengths, uint64_t max_mismatch, uint64_t three_prime);
void win_begin(sw_windows &w, int device, const uint64_t *offsets, uint64_t nq, uint64_t n_groups, const uint32_t *lengths, uint64_t n_lengths,
               uint64_t max_mismatch, uint64_t three_prime);
void win_finish(sw_windows &w, const sw_pileup &p, double walk_ms);

// local.hip: the nine figures of n valid pairs (device list) under scoring system sc, written at the pair's out index; every side
// of a pair is below 2^16 (the callers check it on the host).  st is added to.
void check_scoring(const char *what, const sw_scoring *sc);
void local_device(const Runs &t, const QueryPack &P, const sw_infix_pair *d_pairs, const uint32_t *d_out_idx, uint64_t n, const sw_scoring &sc,
                  uint32_t *const out[LOCAL_FIELDS], LocalStats &st);

namespace {

constexpr hipStream_t HIT_STREAM = SQ_STREAM;

inline Runs runs_of(const RunTable &t) { return Runs{t.packed, t.rec_base, t.rec_len, t.rec_run_off, t.run_pos, t.run_len, t.n_records}; }
inline RunTable table_of(const Runs &r) { return RunTable{r.packed, r.rec_base, r.rec_len, r.rec_run_off, r.run_pos, r.run_len, r.n_records}; }

// bit i set: base g + i of the stream is valid, i < cnt <= 32 (the plane has a word behind its last)
__device__ __forceinline__ uint32_t plane32(const uint32_t *__restrict__ valid, uint64_t g, uint32_t cnt)
{
    const uint64_t w = g >> 5;
    const uint32_t sh = (uint32_t)(g & 31);
    uint64_t x = valid[w];
    if (sh + cnt > 32) x |= (uint64_t)valid[w + 1] << 32;
    x >>= sh;
    return (uint32_t)x & (cnt >= 32 ? 0xFFFFFFFFu : (1u << cnt) - 1);
}

}  // namespace
}  // namespace sw

struct sw_pileup {
    int device = 0;
    uint64_t nq = 0, n_groups = 0;
    std::vector<uint64_t> off;                     // [nq + 1]: the rows of query q are [off[q], off[q + 1])
    sw::DevArray<uint32_t> table, depth;
    sw::DevArray<uint8_t> labels;
    sw::DevArray<unsigned long long> stat;
    sw::PileSink sink{};
    uint64_t counters[5] = {};                     // pairs piled, filtered by distance, left out by label, adds issued, table bytes
    double ms = 0;                                 // the pile walk
};

struct sw_windows {
    int device = 0;
    uint64_t nq = 0, n_groups = 0, n_lengths = 0, max_mismatch = 0, three_prime = 0;
    uint32_t lengths[sw::WIN_MAX_LENGTHS] = {};
    std::vector<uint64_t> off;                     // [nq + 1]: the rows of query q are [off[q], off[q + 1])
    sw::DevArray<uint32_t> table;
    sw::DevArray<uint64_t> d_off;                  // off on the device, for the finishing pass
    sw::DevArray<unsigned long long> stat;
    sw::WinSink sink{};
    uint64_t counters[3] = {};                     // windows visited, adds issued, table bytes
    double ms[2] = {};                             // the window walk, the finishing kernel
};

struct sw_hits {
    int device = 0;
    uint64_t nq = 0, n_asm = 0, k = 0, n_seeds_total = 0;
    std::vector<uint32_t> n_seeds;                 // [nq]
    sw::DevArray<uint32_t> field[5];               // [nq][n_asm] seeds, record, strand, end, dist
    uint64_t counters[10] = {};
    uint64_t seed_counters[8] = {};                // sw_hits_seed_stats
    double ms[4] = {};
    std::vector<uint64_t> chunk_hits;
    bool aligned = false;                          // made by sw_batch_best_hits_aligned
    sw::DevArray<uint32_t> afield[4];              // [nq][n_asm] a_start, nident, mismatch, gaps (aligned only)
    sw::AlignStats align;
    bool has_loci = false;                         // made by sw_batch_best_hits_loci
    sw::HitLoci loci;
    bool has_local = false;                        // made by sw_batch_best_hits_local
    sw::DevArray<uint32_t> lfield[sw::LOCAL_FIELDS];   // [nq][n_asm] the local alignment's nine figures (local only)
    sw::LocalStats local;
};
