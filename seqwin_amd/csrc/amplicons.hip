// amplicons.hip -- the products of primer pairs, and the probes inside them, over the finished site list of an oligo search: which
// pair makes how many products in which assembly, and how many of them a probe detects.  It reads a sw_oligos made with the site
// list (oligo_result.hpp) and never the batch.
//
// It has no counterpart in the reference and is not an in-silico PCR tool (no thermodynamics of its own, no extension model).
// DESIGN.md section 3.2p is the specification, exact in integers; tests/tools/amplicons_host.py restates it twice, and wherever a
// call has neither probe nor max_dg the answer is seqwin_amd/oligos.py: amplicons' on the same list.
//
// The list is ascending by (oligo, assembly, record, pos[, end], strand), so the sites of an oligo are one contiguous range and the
// sites of an (oligo, assembly) cell another, bounded by the scan of n_sites.  This stage is binary searches and short dependent
// walks over sorted 32-bit columns: latency-bound.  Nothing but the answer leaves the device.
//
//   items          for pair i the sites of f serve orientation + (slot 2 i), the sites of r orientation - (slot 2 i + 1; empty with
//                  f == r).  The host's prefix over the slots maps an item number back to (pair, orientation, site).
//   k_amp_lane     an item per lane.  A first site on strand 0 that passes the dg filter: two binary searches in the partner's cell
//                  of the same assembly bound the partners whose pos lies in the window the length bounds allow -- keys (record, pos)
//                  --, then a walk over that range tests strand, filter and the true product length.  The probe's first possible
//                  site is searched once per item; per product one more search (a Hamming result: every probe site is L_p long)
//                  or a bounded walk (an edit result: the sites' own ends decide).  One atomicAdd per item and non-zero count into
//                  n_amplicons / n_detected; the item's count goes into a scratch column.  A range above the bound is left to
//   k_amp_wave     a wave per item of the long list (k_amp_collect makes it): lanes over partners, a ballot and a popcount per 64.
//                  A repeat gives one first site hundreds of partners while its neighbours have none.
//   emit           (only with the list) an exclusive scan of the counts places every item; the same two kernels walk again and
//                  write the nine columns -- a product's place follows from the scan and, in the wave, from the ballot: no atomic
//                  decides it.  The emitted order is (pair, orientation, first site, partner), each in the site list's order.
//   order          the list ascending by its first eight columns, ties in the emitted order: six rounds, least column first, of a
//                  keys-only sort (radix.hip through sort_keys64) of `column << 32 | place` -- the place in the low half makes every
//                  round stable -- and one gather.  On a Hamming result each orientation of a cell is already in order and a merge
//                  per cell would do; an edit result's sites share a pos with different ends, so it would not.  Not measured
//                  against each other.
#include "screen_core.hpp"
#include "oligo_result.hpp"

namespace sw {
namespace {

constexpr uint64_t AMP_MAX_PAIRS = 65536, AMP_MAX_PRODUCTS = 1ull << 32;
constexpr uint64_t AMP_LEN_CAP = 1ull << 33;           // a length bound above every product length (positions are 32-bit) stands for any larger one
constexpr uint32_t AMP_NO_PROBE = 0xFFFFFFFFu;
constexpr uint32_t AMP_WAVE_RANGE = 64;                // partners above which an item goes to k_amp_wave: chosen without a measurement
constexpr uint32_t AMP_WAVE_RANGE_MAX = 1u << 20;      // (a lane's count of partners stays far below 2^32 / 64)
constexpr uint32_t AMP_LONG = 0xFFFFFFFFu;             // the scratch column's mark of an item left to k_amp_wave
constexpr int AMP_COLS = 9;                            // pair, assembly, record, start, end, orientation, mm_f, mm_r, n_probe
enum { C_PAIR, C_ASM, C_REC, C_START, C_END, C_ORIENT, C_MMF, C_MMR, C_NPROBE };
enum { T_PARTNERS, T_PRODUCTS, T_DETECTED, T_LONG, T_N };   // the 64-bit totals of a call

struct AmpArgs {
    // the site list
    const uint64_t *keys;
    const uint32_t *s_asm, *s_rec, *s_pos;
    const int32_t *s_dg;             // nullptr: no filter
    const uint32_t *cell_off;        // [n_oligos * n_asm + 1] the scan of n_sites
    const uint32_t *lens;            // [n_oligos]
    uint64_t n_asm;
    uint32_t edit, d;                // an edit result and its max_edits (else 0, 0)
    int32_t max_dg;
    // the call
    const uint32_t *pairs, *probes;  // [n_pairs][2]; [n_pairs] or nullptr
    const uint64_t *slot_off;        // [2 n_pairs + 1] items before slot 2 pair + orientation
    uint32_t n_slots;
    uint64_t min_len, max_len;       // (at most AMP_LEN_CAP)
    uint32_t wave_range;
    uint32_t *n_amp, *n_det;         // [n_pairs][n_asm]
    uint32_t *counts;                // [items] products of the item; AMP_LONG between k_amp_lane and k_amp_wave
    unsigned long long *totals;      // [T_N]
    const uint64_t *long_items;      // the items of k_amp_wave
    // the emit pass
    const uint32_t *at;              // [items] products before the item
    uint32_t *col[AMP_COLS];
};

__device__ __forceinline__ uint32_t amp_strand(uint64_t key) { return (uint32_t)(key >> 4) & 1u; }

// mm of a Hamming site, dist = mismatch + gaps of an edit site (oligo.hip: site_columns)
__device__ __forceinline__ uint32_t amp_dist(const AmpArgs &g, uint64_t key)
{
    if (!g.edit) return (uint32_t)key & 15u;
    const uint32_t over = (uint32_t)(key >> 5) & 15u, code = (uint32_t)key & 15u;
    return code % 5 + (over > g.d ? over - g.d : g.d - over) + 2 * (code / 5);
}

// one past the site's last base: pos + L, an edit site's own end
__device__ __forceinline__ uint32_t amp_end(const AmpArgs &g, uint64_t key, uint32_t pos, uint32_t len)
{
    return g.edit ? pos + len - g.d + ((uint32_t)(key >> 5) & 15u) : pos + len;
}

// the first site of [lo, hi) whose (record, pos) is not below (UPPER: is above) `key`
template <bool UPPER> __device__ __forceinline__ uint32_t amp_bound(const AmpArgs &g, uint32_t lo, uint32_t hi, uint64_t key)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint64_t k = (uint64_t)g.s_rec[mid] << 32 | g.s_pos[mid];
        if (UPPER ? k <= key : k < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct AmpItem {
    uint32_t pair, orient, a, rec, pf, end_first, d_first;
    uint32_t q_last, len_last, lo, hi;       // the partners to walk: [lo, hi) of the list (empty: the item makes nothing)
    uint32_t len_probe, p_lo, p_hi;          // with a probe (len_probe != 0): its sites of the assembly from the first at or behind end_first on
};

// item -> what its walk needs.  Every index stays inside the list: the slots' prefix and cell_off are its own scans
__device__ __forceinline__ AmpItem amp_item(const AmpArgs &g, uint64_t item)
{
    AmpItem it{};
    uint32_t s = 0, s_hi = g.n_slots;        // the last slot that starts at or before the item (empty slots lie before it)
    while (s + 1 < s_hi) {
        const uint32_t mid = s + ((s_hi - s) >> 1);
        if (g.slot_off[mid] <= item) s = mid; else s_hi = mid;
    }
    it.pair = s >> 1;
    it.orient = s & 1;
    const uint32_t f = g.pairs[2 * it.pair], r = g.pairs[2 * it.pair + 1];
    const uint32_t q_first = it.orient ? r : f;
    it.q_last = it.orient ? f : r;
    const uint32_t i = g.cell_off[(uint64_t)q_first * g.n_asm] + (uint32_t)(item - g.slot_off[s]);
    const uint64_t key = g.keys[i];
    if (amp_strand(key) != 0) return it;
    if (g.s_dg && g.s_dg[i] > g.max_dg) return it;
    it.a = g.s_asm[i];
    it.rec = g.s_rec[i];
    it.pf = g.s_pos[i];
    it.end_first = amp_end(g, key, it.pf, g.lens[q_first]);
    it.d_first = amp_dist(g, key);
    it.len_last = g.lens[it.q_last];
    // pos of the partner: [pf + max(min_len - L - slack, 0), pf + max_len - L + slack]; the true ends decide inside it
    const int64_t slack = g.d, len = it.len_last;
    const int64_t behind = (int64_t)g.min_len - len - slack, last = (int64_t)it.pf + (int64_t)g.max_len - len + slack;
    const int64_t p_min = (int64_t)it.pf + (behind > 0 ? behind : 0), p_max = last < 0xFFFFFFFFll ? last : 0xFFFFFFFFll;
    if (p_min <= p_max) {
        const uint64_t cell = (uint64_t)it.q_last * g.n_asm + it.a;
        const uint32_t c0 = g.cell_off[cell], c1 = g.cell_off[cell + 1];
        it.lo = amp_bound<false>(g, c0, c1, (uint64_t)it.rec << 32 | (uint64_t)p_min);
        it.hi = amp_bound<true>(g, it.lo, c1, (uint64_t)it.rec << 32 | (uint64_t)p_max);
    }
    const uint32_t qp = g.probes ? g.probes[it.pair] : AMP_NO_PROBE;
    if (qp != AMP_NO_PROBE && it.lo < it.hi) {
        const uint64_t cell = (uint64_t)qp * g.n_asm + it.a;
        it.len_probe = g.lens[qp];
        it.p_hi = g.cell_off[cell + 1];
        it.p_lo = amp_bound<false>(g, g.cell_off[cell], it.p_hi, (uint64_t)it.rec << 32 | it.end_first);
    }
    return it;
}

struct AmpProduct {
    uint32_t end, d_last, n_probe;
};

// is partner j of the item's range a product?
__device__ __forceinline__ bool amp_test(const AmpArgs &g, const AmpItem &it, uint32_t j, AmpProduct &p)
{
    const uint64_t key = g.keys[j];
    if (amp_strand(key) != 1) return false;
    if (g.s_dg && g.s_dg[j] > g.max_dg) return false;
    const uint32_t pos_last = g.s_pos[j];            // (>= pf, same record: the range's bounds)
    p.end = amp_end(g, key, pos_last, it.len_last);
    const uint64_t len = (uint64_t)p.end - it.pf;
    if (len < g.min_len || len > g.max_len) return false;
    p.d_last = amp_dist(g, key);
    p.n_probe = 0;
    if (!it.len_probe) return true;
    // probe sites of the record with end_first <= pos_p and end_p <= pos_last
    if (!g.edit) {
        if (pos_last >= it.len_probe) p.n_probe = amp_bound<true>(g, it.p_lo, it.p_hi, (uint64_t)it.rec << 32 | (pos_last - it.len_probe)) - it.p_lo;
    } else {
        const uint32_t shortest = it.len_probe - g.d;   // a site of the probe spans L_p - d bases or more
        for (uint32_t k = it.p_lo; k < it.p_hi && g.s_rec[k] == it.rec && (uint64_t)g.s_pos[k] + shortest <= pos_last; ++k)
            p.n_probe += amp_end(g, g.keys[k], g.s_pos[k], it.len_probe) <= pos_last;
    }
    return true;
}

__device__ __forceinline__ void amp_write(const AmpArgs &g, const AmpItem &it, const AmpProduct &p, uint32_t at)
{
    g.col[C_PAIR][at] = it.pair;
    g.col[C_ASM][at] = it.a;
    g.col[C_REC][at] = it.rec;
    g.col[C_START][at] = it.pf;
    g.col[C_END][at] = p.end;
    g.col[C_ORIENT][at] = it.orient;
    g.col[C_MMF][at] = it.orient ? p.d_last : it.d_first;
    g.col[C_MMR][at] = it.orient ? it.d_first : p.d_last;
    g.col[C_NPROBE][at] = p.n_probe;
}

__device__ __forceinline__ uint32_t amp_wave_sum(uint32_t v)
{
    for (uint32_t d = SCR_WAVE / 2; d; d >>= 1) v += __shfl_xor(v, d, SCR_WAVE);
    return v;
}

// what an item adds to its cell and to the call
__device__ __forceinline__ void amp_count(const AmpArgs &g, const AmpItem &it, uint32_t n, uint32_t detected)
{
    if (n) atomicAdd(g.n_amp + (uint64_t)it.pair * g.n_asm + it.a, n);
    if (detected) atomicAdd(g.n_det + (uint64_t)it.pair * g.n_asm + it.a, detected);
}

template <bool EMIT> __global__ __launch_bounds__(SCR_TPB) void k_amp_lane(uint64_t base, uint64_t end, AmpArgs g)
{
    const uint64_t item = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    uint32_t n = 0, detected = 0, visited = 0, is_long = 0;
    if (item < end) {
        const AmpItem it = amp_item(g, item);
        if (it.hi - it.lo > g.wave_range) {
            is_long = 1;
        } else {
            uint32_t at = EMIT ? g.at[item] : 0;
            for (uint32_t j = it.lo; j < it.hi; ++j) {
                AmpProduct p;
                if (!amp_test(g, it, j, p)) continue;
                if (EMIT) amp_write(g, it, p, at++);
                ++n;
                detected += p.n_probe != 0;
            }
            visited = it.hi - it.lo;
            if (!EMIT) amp_count(g, it, n, detected);
        }
        if (!EMIT) g.counts[item] = is_long ? AMP_LONG : n;
    }
    if (EMIT) return;
    // (the whole wave)
    const uint32_t sums[T_N] = {amp_wave_sum(visited), amp_wave_sum(n), amp_wave_sum(detected), amp_wave_sum(is_long)};
    if (threadIdx.x % SCR_WAVE == 0)
        for (int t = 0; t < T_N; ++t)
            if (sums[t]) atomicAdd(g.totals + t, (unsigned long long)sums[t]);
}

// the marked items of [base, end) -> the long list, in no particular order: every item's results have a place of their own
__global__ __launch_bounds__(SCR_TPB) void k_amp_collect(uint64_t base, uint64_t end, const uint32_t *__restrict__ counts, uint64_t *__restrict__ list,
                                                         unsigned long long cap, unsigned long long *cursor)
{
    const uint64_t item = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    const uint32_t mine = item < end && counts[item] == AMP_LONG;
    const WaveRange w = wave_append(cursor, threadIdx.x % SCR_WAVE, mine);
    if (mine && w.base + w.offset < cap) list[w.base + w.offset] = item;
}

// entry e of the long list: a wave over the item's partners, 64 at a time
template <bool EMIT> __global__ __launch_bounds__(SCR_TPB) void k_amp_wave(uint64_t base, uint64_t end, AmpArgs g)
{
    const uint32_t lane = threadIdx.x % SCR_WAVE;
    const uint64_t e = base + (uint64_t)blockIdx.x * SCR_WPB + threadIdx.x / SCR_WAVE;
    if (e >= end) return;                    // (the whole wave)
    const uint64_t item = g.long_items[e];
    const AmpItem it = amp_item(g, item);    // (uniform)
    const uint32_t at = EMIT ? g.at[item] : 0;
    uint32_t n = 0, detected = 0;
    for (uint64_t j0 = it.lo; j0 < it.hi; j0 += SCR_WAVE) {   // (uniform)
        const uint64_t j = j0 + lane;
        AmpProduct p{};
        const bool ok = j < it.hi && amp_test(g, it, (uint32_t)j, p);
        const unsigned long long m = __ballot(ok), md = __ballot(ok && p.n_probe != 0);
        if (EMIT && ok) amp_write(g, it, p, at + n + (uint32_t)__popcll(m & ((1ull << lane) - 1)));
        n += (uint32_t)__popcll(m);
        detected += (uint32_t)__popcll(md);
    }
    if (EMIT || lane) return;
    g.counts[item] = n;
    amp_count(g, it, n, detected);
    atomicAdd(g.totals + T_PARTNERS, (unsigned long long)(it.hi - it.lo));
    if (n) atomicAdd(g.totals + T_PRODUCTS, (unsigned long long)n);
    if (detected) atomicAdd(g.totals + T_DETECTED, (unsigned long long)detected);
}

// ---- the order of the list ------------------------------------------------------------------------------------------------------
struct AmpCols {
    const uint32_t *col[AMP_COLS];
};

// round -> the 32 bits it orders by, least first: (orientation, mm_f, mm_r), end, start, record, assembly, pair
__device__ __forceinline__ uint32_t amp_round_field(const AmpCols &c, uint32_t round, uint32_t i)
{
    switch (round) {
    case 0: return c.col[C_ORIENT][i] << 8 | c.col[C_MMF][i] << 4 | c.col[C_MMR][i];   // (a dist is at most 8)
    case 1: return c.col[C_END][i];
    case 2: return c.col[C_START][i];
    case 3: return c.col[C_REC][i];
    case 4: return c.col[C_ASM][i];
    default: return c.col[C_PAIR][i];
    }
}
constexpr uint32_t AMP_ROUNDS = 6;

// keys[i] = the round's field of the product now at place i, above i.  perm: place -> emitted index (nullptr: the identity)
__global__ __launch_bounds__(SCR_TPB) void k_amp_keys(uint64_t base, uint64_t end, AmpCols c, uint32_t round, const uint32_t *__restrict__ perm,
                                                      uint64_t *__restrict__ keys)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end) return;
    keys[i] = (uint64_t)amp_round_field(c, round, perm ? perm[i] : (uint32_t)i) << 32 | i;
}

// the sorted keys' low halves are the places before the round
__global__ __launch_bounds__(SCR_TPB) void k_amp_perm(uint64_t base, uint64_t end, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ perm,
                                                      uint32_t *__restrict__ perm_out)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end) return;
    const uint32_t was = (uint32_t)keys[i];
    perm_out[i] = perm ? perm[was] : was;
}

__global__ __launch_bounds__(SCR_TPB) void k_amp_gather(uint64_t base, uint64_t end, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ src,
                                                        uint32_t *__restrict__ dst)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end) return;
    dst[i] = src[perm[i]];
}

// kern(base, end, args ...) over [0, n) units, `per_block` of them a workgroup, in launches of at most blocks_max workgroups
template <class K, class... A> uint64_t amp_launch(K kern, uint64_t n, uint32_t per_block, uint32_t blocks_max, hipStream_t stream, A... args)
{
    const uint64_t per = (uint64_t)blocks_max * per_block;
    uint64_t launches = 0;
    for (uint64_t base = 0; base < n; base += per, ++launches) {
        const uint64_t cnt = std::min<uint64_t>(per, n - base);
        hipLaunchKernelGGL(kern, dim3((unsigned)((cnt + per_block - 1) / per_block)), dim3(SCR_TPB), 0, stream, base, base + cnt, args...);
        SW_HIP(hipGetLastError());
    }
    return launches;
}

}  // namespace
}  // namespace sw

struct sw_amplicons {
    int device = 0;
    uint64_t n_pairs = 0, n_asm = 0, min_len = 0, max_len = 0;
    bool has_products = false;
    uint64_t n_products = 0;
    sw::DevArray<uint32_t> n_amp, n_det;     // [n_pairs][n_asm]
    sw::DevArray<uint32_t> col[sw::AMP_COLS]; // [n_products] the list, in its final order
    uint64_t counters[6] = {};               // items, items on the wave route, partners visited, products, detected products, launches
    double ms[3] = {};                       // count, emit, order
};

namespace sw {
namespace {

// what a call says about itself, before a device is touched
void check_amplicons(const sw_oligos *o, const uint32_t *pairs, const uint32_t *probes, uint64_t n_pairs, uint64_t min_len, uint64_t max_len, bool filter,
                     sw_amplicons **out)
{
    if (!o || !out) raise(SW_ERR_VALUE, "amplicons: a NULL handle or array");
    if (n_pairs < 1 || n_pairs > AMP_MAX_PAIRS) raise(SW_ERR_VALUE, "amplicons: %llu pairs; 1..%llu are taken", (unsigned long long)n_pairs, (unsigned long long)AMP_MAX_PAIRS);
    if (!pairs) raise(SW_ERR_VALUE, "amplicons: a NULL handle or array");
    if (!o->has_sites) raise(SW_ERR_VALUE, "amplicons: these oligo hits were made without the site list");
    if (filter && !o->thermo) raise(SW_ERR_VALUE, "amplicons: max_dg needs oligo hits made with a thermodynamic model");
    if (min_len < 1) raise(SW_ERR_VALUE, "amplicons: min_len must be 1 or more");
    if (min_len > max_len) raise(SW_ERR_VALUE, "amplicons: min_len %llu exceeds max_len %llu", (unsigned long long)min_len, (unsigned long long)max_len);
    for (uint64_t i = 0; i < n_pairs; ++i) {
        for (int s = 0; s < 2; ++s)
            if (pairs[2 * i + s] >= o->nq)
                raise(SW_ERR_VALUE, "amplicons: pair %llu names oligo %u; the call had %llu", (unsigned long long)i, pairs[2 * i + s], (unsigned long long)o->nq);
        if (probes && probes[i] != AMP_NO_PROBE && probes[i] >= o->nq)
            raise(SW_ERR_VALUE, "amplicons: the probe of pair %llu is oligo %u; the call had %llu", (unsigned long long)i, probes[i], (unsigned long long)o->nq);
    }
}

unsigned long long read_totals(const DevArray<unsigned long long> &d, unsigned long long *t, hipStream_t stream)
{
    SW_HIP(hipMemcpyAsync(t, d.p, T_N * 8, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    return t[T_PRODUCTS];
}

void oligos_amplicons(const sw_oligos &o, const uint32_t *pairs, const uint32_t *probes, uint64_t n_pairs, uint64_t min_len, uint64_t max_len, bool want_products,
                      bool filter, int32_t max_dg, hipStream_t stream, sw_amplicons &r)
{
    const uint64_t nq = o.nq, n_asm = o.n_asm, cells = nq * n_asm, out_cells = n_pairs * n_asm;
    r.n_pairs = n_pairs;
    r.n_asm = n_asm;
    r.min_len = min_len;
    r.max_len = max_len;
    r.has_products = want_products;
    r.n_amp.alloc(out_cells);
    r.n_det.alloc(out_cells);
    if (out_cells) {
        SW_HIP(hipMemsetAsync(r.n_amp.p, 0, out_cells * 4, stream));
        SW_HIP(hipMemsetAsync(r.n_det.p, 0, out_cells * 4, stream));
    }
    uint32_t wave_range = AMP_WAVE_RANGE;
    if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_AMP_WAVE_RANGE")) wave_range = (uint32_t)std::min<uint64_t>(env_u64(e, wave_range), AMP_WAVE_RANGE_MAX);
    const uint32_t blocks_max = launch_blocks("SEQWIN_AMD_AMP_MAX_BLOCKS");
    // ---- the scan of n_sites, and from it the sites of every oligo ----
    DevArray<uint32_t> cell_off(cells + 1);
    SW_HIP(hipMemsetAsync(cell_off.p, 0, 4, stream));
    std::vector<uint32_t> oligo_off(nq + 1, 0);
    if (cells && o.n_list) {
        size_t tmp_bytes = 0;
        SW_HIP(rocprim::inclusive_scan(nullptr, tmp_bytes, o.field[0].p, cell_off.p + 1, cells, rocprim::plus<uint32_t>(), stream));
        DevArray<unsigned char> tmp(tmp_bytes);
        SW_HIP(rocprim::inclusive_scan(tmp.p, tmp_bytes, o.field[0].p, cell_off.p + 1, cells, rocprim::plus<uint32_t>(), stream));
        SW_HIP(hipMemcpy2DAsync(oligo_off.data(), 4, cell_off.p, n_asm * 4, 4, nq, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
        oligo_off[nq] = (uint32_t)o.n_list;      // (below 2^32: oligo.hip refuses a longer list)
    }
    std::vector<uint64_t> slot_off(2 * n_pairs + 1, 0);
    for (uint64_t i = 0; i < n_pairs; ++i) {
        const uint32_t f = pairs[2 * i], b = pairs[2 * i + 1];
        slot_off[2 * i + 1] = slot_off[2 * i] + (oligo_off[f + 1] - oligo_off[f]);
        slot_off[2 * i + 2] = slot_off[2 * i + 1] + (f == b ? 0 : oligo_off[b + 1] - oligo_off[b]);   // with f == r only + is formed
    }
    const uint64_t items = slot_off.back();
    uint64_t launches = 0;
    unsigned long long tot[T_N] = {};
    Event e0, e1, e2, e3;
    SW_HIP(hipEventRecord(e0, stream));
    // what the passes share (declared here: the emit pass reads them again)
    DevArray<uint32_t> d_lens(nq), d_pairs(2 * n_pairs), d_probes, counts, at;
    DevArray<uint64_t> d_slot_off(slot_off.size()), long_items;
    DevArray<unsigned long long> totals(T_N), cursor(1);
    AmpArgs g{};
    if (items) {
        SW_HIP(hipMemcpyAsync(d_lens.p, o.lens.data(), nq * 4, hipMemcpyHostToDevice, stream));
        SW_HIP(hipMemcpyAsync(d_pairs.p, pairs, n_pairs * 8, hipMemcpyHostToDevice, stream));
        SW_HIP(hipMemcpyAsync(d_slot_off.p, slot_off.data(), slot_off.size() * 8, hipMemcpyHostToDevice, stream));
        if (probes) {
            d_probes.alloc(n_pairs);
            SW_HIP(hipMemcpyAsync(d_probes.p, probes, n_pairs * 4, hipMemcpyHostToDevice, stream));
        }
        SW_HIP(hipMemsetAsync(totals.p, 0, T_N * 8, stream));
        counts.alloc(items);
        g.keys = o.keys.p;
        g.s_asm = o.s_asm.p;
        g.s_rec = o.s_rec.p;
        g.s_pos = o.s_pos.p;
        g.s_dg = filter ? o.s_sum[2].p : nullptr;
        g.cell_off = cell_off.p;
        g.lens = d_lens.p;
        g.n_asm = n_asm;
        g.edit = o.max_edits >= 0;
        g.d = g.edit ? (uint32_t)o.max_edits : 0;
        g.max_dg = max_dg;
        g.pairs = d_pairs.p;
        g.probes = d_probes.p;
        g.slot_off = d_slot_off.p;
        g.n_slots = (uint32_t)(2 * n_pairs);
        g.min_len = std::min(min_len, AMP_LEN_CAP);
        g.max_len = std::min(max_len, AMP_LEN_CAP);
        g.wave_range = wave_range;
        g.n_amp = r.n_amp.p;
        g.n_det = r.n_det.p;
        g.counts = counts.p;
        g.totals = totals.p;
        // ---- the count pass ----
        launches += amp_launch(k_amp_lane<false>, items, SCR_TPB, blocks_max, stream, g);
        read_totals(totals, tot, stream);
        if (tot[T_LONG]) {
            long_items.alloc(tot[T_LONG]);
            SW_HIP(hipMemsetAsync(cursor.p, 0, 8, stream));
            launches += amp_launch(k_amp_collect, items, SCR_TPB, blocks_max, stream, (const uint32_t *)counts.p, long_items.p, tot[T_LONG], cursor.p);
            g.long_items = long_items.p;
            launches += amp_launch(k_amp_wave<false>, tot[T_LONG], SCR_WPB, blocks_max, stream, g);
            read_totals(totals, tot, stream);
        }
        if (tot[T_PRODUCTS] >= AMP_MAX_PRODUCTS) raise(SW_ERR_RUNTIME, "amplicons: the call has 2^32 products or more");
    }
    const uint64_t n_products = tot[T_PRODUCTS];
    SW_HIP(hipEventRecord(e1, stream));
    // ---- the emit pass: an item's place is the scan of the counts ----
    DevArray<uint32_t> emitted[AMP_COLS];
    if (want_products && n_products) {
        at.alloc(items);
        size_t tmp_bytes = 0;
        SW_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, counts.p, at.p, uint32_t(0), items, rocprim::plus<uint32_t>(), stream));
        DevArray<unsigned char> tmp(tmp_bytes);
        SW_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, counts.p, at.p, uint32_t(0), items, rocprim::plus<uint32_t>(), stream));
        g.at = at.p;
        for (int c = 0; c < AMP_COLS; ++c) {
            emitted[c].alloc(n_products);
            g.col[c] = emitted[c].p;
        }
        launches += amp_launch(k_amp_lane<true>, items, SCR_TPB, blocks_max, stream, g);
        if (tot[T_LONG]) launches += amp_launch(k_amp_wave<true>, tot[T_LONG], SCR_WPB, blocks_max, stream, g);
    }
    SW_HIP(hipEventRecord(e2, stream));
    // ---- the order: six stable rounds, least column first ----
    if (want_products && n_products) {
        AmpCols cols;
        for (int c = 0; c < AMP_COLS; ++c) cols.col[c] = emitted[c].p;
        DevArray<uint64_t> ka(n_products), kb(n_products);
        DevArray<uint32_t> pa(n_products), pb(n_products);
        const uint32_t *perm = nullptr;
        uint32_t *next = pa.p, *other = pb.p;
        for (uint32_t round = 0; round < AMP_ROUNDS; ++round) {
            uint64_t *kp = ka.p, *ap = kb.p;
            launches += amp_launch(k_amp_keys, n_products, SCR_TPB, blocks_max, stream, cols, round, perm, kp);
            sort_all_bits(kp, ap, n_products, stream);
            launches += amp_launch(k_amp_perm, n_products, SCR_TPB, blocks_max, stream, (const uint64_t *)kp, perm, next);
            perm = next;
            std::swap(next, other);
        }
        for (int c = 0; c < AMP_COLS; ++c) {
            r.col[c].alloc(n_products);
            launches += amp_launch(k_amp_gather, n_products, SCR_TPB, blocks_max, stream, perm, (const uint32_t *)emitted[c].p, r.col[c].p);
        }
    }
    r.n_products = n_products;
    SW_HIP(hipEventRecord(e3, stream));
    SW_HIP(hipStreamSynchronize(stream));   // (the temporaries go back to the pool behind the kernels)
    const hipEvent_t ev[4] = {e0, e1, e2, e3};
    for (int i = 0; i < 3; ++i) {
        float ms = 0;
        SW_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        r.ms[i] = i == 0 || (want_products && n_products) ? ms : 0;   // (without a list nothing is emitted or ordered)
    }
    r.counters[0] = items;
    r.counters[1] = tot[T_LONG];
    r.counters[2] = tot[T_PARTNERS];
    r.counters[3] = n_products;
    r.counters[4] = tot[T_DETECTED];
    r.counters[5] = launches;
}

}  // namespace
}  // namespace sw

using namespace sw;

extern "C" {

int sw_oligos_amplicons(const sw_oligos *oligos, const uint32_t *pairs, const uint32_t *probes, uint64_t n_pairs, uint64_t min_len, uint64_t max_len,
                        int want_products, int64_t max_dg, int no_threshold, void *stream, sw_amplicons **out)
{
    return guarded([&] {
        check_amplicons(oligos, pairs, probes, n_pairs, min_len, max_len, !no_threshold, out);
        require_device(oligos->device, "the oligo hits");
        StreamScope scope((hipStream_t)stream);
        std::unique_ptr<sw_amplicons> r(new sw_amplicons);
        r->device = oligos->device;
        const int32_t dg = (int32_t)std::min<int64_t>(std::max<int64_t>(max_dg, INT32_MIN), INT32_MAX);
        oligos_amplicons(*oligos, pairs, probes, n_pairs, min_len, max_len, want_products != 0, !no_threshold, dg, (hipStream_t)stream, *r);
        *out = r.release();
    });
}

int sw_amplicons_sizes(const sw_amplicons *h, uint64_t *n_pairs, uint64_t *n_assemblies, uint64_t *min_len, uint64_t *max_len)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "amplicons: a NULL handle");
        if (n_pairs) *n_pairs = h->n_pairs;
        if (n_assemblies) *n_assemblies = h->n_asm;
        if (min_len) *min_len = h->min_len;
        if (max_len) *max_len = h->max_len;
    });
}

int sw_amplicons_block(const sw_amplicons *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "amplicons: a NULL handle");
        if (field > 1) raise(SW_ERR_VALUE, "amplicons: field %llu; 0 n_amplicons, 1 n_detected", (unsigned long long)field);
        export_cells("amplicons", "pairs", h->device, "the amplicons", field ? h->n_det.p : h->n_amp.p, h->n_pairs, h->n_asm, r0, r1, c0, c1, out);
    });
}

int sw_amplicons_products_size(const sw_amplicons *h, uint64_t *n_products)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "amplicons: a NULL handle");
        if (!h->has_products) raise(SW_ERR_VALUE, "amplicons: these amplicons were made without the list of products");
        if (n_products) *n_products = h->n_products;
    });
}

int sw_amplicons_products(const sw_amplicons *h, uint64_t *cell_offsets, uint32_t *pair, uint32_t *assembly, uint32_t *record, uint32_t *start, uint32_t *end,
                          uint32_t *orientation, uint32_t *mm_f, uint32_t *mm_r, uint32_t *n_probe)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "amplicons: a NULL handle");
        if (!h->has_products) raise(SW_ERR_VALUE, "amplicons: these amplicons were made without the list of products");
        uint32_t *dst[AMP_COLS] = {pair, assembly, record, start, end, orientation, mm_f, mm_r, n_probe};
        const uint64_t n = h->n_products, cells = h->n_pairs * h->n_asm;
        if (!cell_offsets) raise(SW_ERR_VALUE, "amplicons: a NULL handle or array");
        for (int c = 0; c < AMP_COLS; ++c)
            if (n && !dst[c]) raise(SW_ERR_VALUE, "amplicons: a NULL handle or array");
        require_device(h->device, "the amplicons");
        std::vector<uint32_t> counts(cells);
        if (cells) SW_HIP(hipMemcpy(counts.data(), h->n_amp.p, cells * 4, hipMemcpyDeviceToHost));
        cell_offsets[0] = 0;
        for (uint64_t c = 0; c < cells; ++c) cell_offsets[c + 1] = cell_offsets[c] + counts[c];
        if (cell_offsets[cells] != n) raise(SW_ERR_RUNTIME, "internal error: the cells' product counts do not add up to the list");
        for (int c = 0; c < AMP_COLS && n; ++c) SW_HIP(hipMemcpy(dst[c], h->col[c].p, n * 4, hipMemcpyDeviceToHost));
    });
}

int sw_amplicons_stats(const sw_amplicons *h, uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "amplicons: a NULL handle");
        if (counters) memcpy(counters, h->counters, sizeof h->counters);
        if (ms) memcpy(ms, h->ms, sizeof h->ms);
    });
}

void sw_amplicons_free(sw_amplicons *h)
{
    delete h;
}

}  // extern "C"
