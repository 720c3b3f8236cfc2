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
//   k_scr_probe    the hot path.  The run / tile / lane walk of k_mh_hash (minhash.hip): a tile of 1024 k-mers of one valid run per
//                  wave, 16 consecutive k-mers per lane.  A lane rolls its 16 canonical words, issues their 16 first-slot loads
//                  together, resolves the occupied ones, and sets bit `number` of its assembly's row of a presence bitmap with
//                  atomicOr -- consecutive hits that fall into one bitmap word leave as one atomic
//   k_scr_reduce   counts[q, a] = sum over q's pairs of popcount(bitmap[a][word] & mask): a wave per (query, assembly)
// The bitmap holds a chunk of assemblies (a budget, 1 GiB by default); tiles are ordered by assembly, so a chunk is a tile range.
#include <cstring>  // rocprim's texture iterator needs ::memset declared first
#include <memory>

#include <rocprim/rocprim.hpp>

#include "device.hpp"

namespace sw {
namespace {

constexpr uint32_t SCR_TPB = 256, SCR_WAVE = 64, SCR_WPB = SCR_TPB / SCR_WAVE;
constexpr uint32_t SCR_L = 16;                        // consecutive k-mers per lane
constexpr uint32_t SCR_TILE = SCR_WAVE * SCR_L;       // k-mers per wave: one tile lies inside one valid run
constexpr uint32_t SCR_MAX_BLOCKS = 1u << 22;         // workgroups per launch: 2^30 threads, below the 2^32 a launch may hold
constexpr uint64_t SCR_MAX_TEXT = 0xFFFFFFFFull - 255; // query text: fewer bytes than this (a thread per byte in workgroups of 256)
constexpr uint64_t SCR_MAX_DISTINCT = 1ull << 31;     // distinct query k-mers: fewer than this (a slot holds number + 1 in 32 bits)
constexpr uint64_t SCR_BITMAP_BYTES = 1ull << 30;     // budget of the presence bitmap: speed only, chosen without a measurement
constexpr uint32_t SCR_RED_ROWS = 64;                 // assemblies per workgroup of k_scr_reduce (16 per wave)
constexpr uint32_t SCR_NONE = 0xFFFFFFFFu;

uint64_t scr_env_u64(const char *v, uint64_t dflt)
{
    if (!v || !*v) return dflt;
    char *end = nullptr;
    const unsigned long long x = strtoull(v, &end, 10);
    return (end && *end == 0) ? (uint64_t)x : dflt;
}

// workgroups per launch; SEQWIN_AMD_SCR_MAX_BLOCKS (test library) lowers it so that a small input needs several launches
uint32_t scr_launch_blocks()
{
    return (uint32_t)std::max<uint64_t>(std::min<uint64_t>(scr_env_u64(SW_TEST_GETENV("SEQWIN_AMD_SCR_MAX_BLOCKS"), SCR_MAX_BLOCKS), SCR_MAX_BLOCKS), 1);
}

void scr_require_device(int device, const char *what)
{
    int cur = -1;
    SW_HIP(hipGetDevice(&cur));
    if (cur != device)
        raise(SW_ERR_VALUE, "%s lives on device %d but the calling thread's current device is %d (sw_set_device)", what, device, cur);
}

// ---- the table ------------------------------------------------------------------------------------------------------------------
// Open addressing over `cap` = 2^bits slots, linear probing.  A slot holds (index into keys) + 1, 0 = empty; keys are distinct.
struct Table {
    const uint32_t *slots;
    const uint64_t *keys;
    uint64_t cap;
    uint32_t bits;
};

__host__ __device__ __forceinline__ uint32_t scr_home(uint64_t key, uint32_t bits)
{
    return bits ? (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - bits)) : 0u;
}

// index of `key`, SCR_NONE if it is not in the table; s0: what the key's home slot holds
__device__ __forceinline__ uint32_t scr_find_from(const Table &t, uint64_t key, uint32_t h, uint32_t s)
{
    const uint32_t mask = (uint32_t)(t.cap - 1);
    for (uint64_t n = 0; n < t.cap; ++n) {   // (bounded by the capacity: a full circle ends the search)
        if (!s) return SCR_NONE;
        if (t.keys[s - 1] == key) return s - 1;
        h = (h + 1) & mask;
        s = t.slots[h];
    }
    return SCR_NONE;
}

__device__ __forceinline__ uint32_t scr_find(const Table &t, uint64_t key)
{
    const uint32_t h = scr_home(key, t.bits);
    return scr_find_from(t, key, h, t.slots[h]);
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (uint32_t d = SCR_WAVE / 2; d; d >>= 1) {
        const uint32_t o = __shfl_down(v, d, SCR_WAVE);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (uint32_t d = SCR_WAVE / 2; d; d >>= 1) v += __shfl_down(v, d, SCR_WAVE);
    return v;
}

// Every key claims the first empty slot from its home on.  The keys are distinct, so nothing is compared and no thread waits for
// another: a lost atomicCAS moves on.  chain: the most slots a key visited; fail: a key found no slot (cannot happen below capacity)
__global__ __launch_bounds__(SCR_TPB) void k_scr_insert(uint64_t base, uint64_t end, const uint64_t *__restrict__ keys, uint32_t *__restrict__ slots,
                                                        uint64_t cap, uint32_t bits, uint32_t *__restrict__ chain, uint32_t *__restrict__ fail)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    uint32_t visited = 0;
    if (i < end) {
        const uint32_t mask = (uint32_t)(cap - 1);
        uint32_t h = scr_home(keys[i], bits);
        bool placed = false;
        for (uint64_t n = 0; n < cap && !placed; ++n) {
            placed = atomicCAS(slots + h, 0u, (uint32_t)i + 1) == 0u;
            h = (h + 1) & mask;
            ++visited;
        }
        if (!placed) atomicOr(fail, 1u);
    }
    visited = wave_max(visited);
    if (threadIdx.x % SCR_WAVE == 0 && visited) atomicMax(chain, visited);
}

// ---- query side -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t base_code(uint8_t c)
{
    switch (c | 0x20) {   // ACGTU in either case; U reads as T; every other byte is invalid
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': case 'u': return 3;
    default: return 4;
    }
}

// the last q with off[q] <= p (p < off[nq]: the query that holds byte p; empty queries are stepped over)
__device__ __forceinline__ uint32_t query_of(const uint64_t *__restrict__ off, uint32_t nq, uint64_t p)
{
    uint32_t lo = 0, hi = nq;
    while (lo + 1 < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// word[p] / ok[p]: the canonical word of the k bytes from p on, if they lie inside one query and are all valid
__global__ __launch_bounds__(SCR_TPB) void k_scr_qwords(uint64_t base, uint64_t end, const uint8_t *__restrict__ text, const uint64_t *__restrict__ off,
                                                        uint32_t nq, uint32_t k, uint64_t *__restrict__ word, uint8_t *__restrict__ ok)
{
    const uint64_t p = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (p >= end) return;
    const uint64_t q_end = off[query_of(off, nq, p) + 1];
    bool valid = p + k <= q_end;
    uint64_t fwd = 0, rev = 0;
    if (valid) {
        const uint32_t sh = 2 * (k - 1);
        for (uint32_t i = 0; i < k; ++i) {
            const uint64_t c = base_code(text[p + i]);
            if (c > 3) {
                valid = false;
                break;
            }
            fwd = (fwd << 2) | c;                 // first base most significant (k = 32 fills the word)
            rev = (rev >> 2) | ((3 - c) << sh);
        }
    }
    word[p] = fwd < rev ? fwd : rev;
    ok[p] = valid ? 1 : 0;
}

struct FlagAt {
    const uint8_t *f;
    uint64_t n;
    __host__ __device__ uint32_t operator()(uint64_t i) const { return i < n ? (uint32_t)f[i] : 0u; }
};

// the flagged elements, in order: out_word[at[i]] = word[i], out_pos[at[i]] = i
__global__ __launch_bounds__(SCR_TPB) void k_scr_compact(uint64_t base, uint64_t end, const uint8_t *__restrict__ flag, const uint32_t *__restrict__ at,
                                                         const uint64_t *__restrict__ word, uint64_t *__restrict__ out_word, uint32_t *__restrict__ out_pos)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end || !flag[i]) return;
    out_word[at[i]] = word[i];
    if (out_pos) out_pos[at[i]] = (uint32_t)i;
}

__global__ __launch_bounds__(SCR_TPB) void k_scr_heads(uint64_t base, uint64_t end, const uint64_t *__restrict__ sorted, uint32_t shift, uint8_t *__restrict__ flag)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i < end) flag[i] = (i == 0 || (sorted[i] >> shift) != (sorted[i - 1] >> shift)) ? 1 : 0;
}

// sidx[j] = where valid word j lies among the distinct words; first[that] = the smallest such j
__global__ __launch_bounds__(SCR_TPB) void k_scr_first(uint64_t base, uint64_t end, Table t, const uint64_t *__restrict__ vword, uint32_t *__restrict__ sidx,
                                                       uint32_t *__restrict__ first, uint32_t *__restrict__ fail)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j >= end) return;
    const uint32_t s = scr_find(t, vword[j]);
    sidx[j] = s;
    if (s == SCR_NONE) atomicOr(fail, 2u);
    else atomicMin(first + s, (uint32_t)j);
}

__global__ __launch_bounds__(SCR_TPB) void k_scr_is_first(uint64_t base, uint64_t end, const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ first,
                                                          uint8_t *__restrict__ flag)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j < end) flag[j] = (sidx[j] != SCR_NONE && first[sidx[j]] == (uint32_t)j) ? 1 : 0;
}

// the number of a distinct word = how many distinct words appeared before its first appearance
__global__ __launch_bounds__(SCR_TPB) void k_scr_number(uint64_t base, uint64_t end, const uint8_t *__restrict__ flag, const uint32_t *__restrict__ at,
                                                        const uint32_t *__restrict__ sidx, const uint64_t *__restrict__ vword, uint32_t *__restrict__ number,
                                                        uint64_t *__restrict__ by_number)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j >= end || !flag[j]) return;
    number[sidx[j]] = at[j];
    by_number[at[j]] = vword[j];
}

__global__ __launch_bounds__(SCR_TPB) void k_scr_relabel(uint64_t base, uint64_t end, uint32_t *__restrict__ slots, const uint32_t *__restrict__ number)
{
    const uint64_t h = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (h < end && slots[h]) slots[h] = number[slots[h] - 1] + 1;
}

__global__ __launch_bounds__(SCR_TPB) void k_scr_qkeys(uint64_t base, uint64_t end, const uint32_t *__restrict__ vpos, const uint32_t *__restrict__ sidx,
                                                       const uint32_t *__restrict__ number, const uint64_t *__restrict__ off, uint32_t nq,
                                                       uint64_t *__restrict__ qkey)
{
    const uint64_t j = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (j < end) qkey[j] = ((uint64_t)query_of(off, nq, vpos[j]) << 32) | number[sidx[j]];
}

// sorted (query << 32 | number): pair `at` of a (query, bitmap word) run gets the word, the OR of the run's bits, and is counted
// for its query; a query's distinct numbers are counted on the way
__global__ __launch_bounds__(SCR_TPB) void k_scr_pairs(uint64_t base, uint64_t end, const uint64_t *__restrict__ qkey, const uint8_t *__restrict__ head,
                                                       const uint32_t *__restrict__ at, uint32_t *__restrict__ pword, uint32_t *__restrict__ pmask,
                                                       uint32_t *__restrict__ n_pairs, uint32_t *__restrict__ n_kmers)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * SCR_TPB + threadIdx.x;
    if (i >= end) return;
    const uint64_t x = qkey[i];
    const uint32_t q = (uint32_t)(x >> 32), id = (uint32_t)x;
    const uint32_t pair = at[i] + head[i] - 1;   // (at: the heads before i; the run's own head lies before i unless i is it)
    if (head[i]) {
        pword[pair] = id >> 5;
        atomicAdd(n_pairs + q, 1u);
    }
    if (i == 0 || qkey[i - 1] != x) {
        atomicOr(pmask + pair, 1u << (id & 31));
        atomicAdd(n_kmers + q, 1u);
    }
}

// ---- probe ----------------------------------------------------------------------------------------------------------------------
struct ProbeArgs {
    const uint32_t *packed;          // 16 bases per word, base i in bits [2 (i % 16), +2)
    const uint64_t *run_base;        // [n_runs] batch-wide index of the run's first base
    const uint32_t *run_nk;          // [n_runs] k-mers of the run (>= 1)
    const uint32_t *run_asm;         // [n_runs]
    const uint32_t *run_tile_off;    // [n_runs + 1] first tile of the run
    uint32_t n_runs;
    uint32_t tile_begin, tile_end;   // the tiles of this launch: all of assemblies [asm0, asm0 + rows of the bitmap)
    Table t;                         // slots hold number + 1, keys are in number order
    uint32_t *bitmap;                // [assembly - asm0][words]
    uint32_t asm0;
    uint64_t words;                  // ceil(distinct / 32)
    unsigned long long *stat;        // [0] hits, [1] atomics issued
    uint32_t k;
};

__global__ __launch_bounds__(SCR_TPB) void k_scr_probe(ProbeArgs g)
{
    const uint32_t wave = threadIdx.x / SCR_WAVE, lane = threadIdx.x % SCR_WAVE;
    const uint64_t tile64 = (uint64_t)g.tile_begin + (uint64_t)blockIdx.x * SCR_WPB + wave;
    if (tile64 >= g.tile_end) return;   // (the whole wave)
    const uint32_t tile = (uint32_t)tile64;
    uint32_t lo = 0, hi = g.n_runs;     // the last run whose first tile is <= tile
    while (lo + 1 < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g.run_tile_off[mid] <= tile) lo = mid; else hi = mid;
    }
    const uint32_t r = lo, nk = g.run_nk[r], a = g.run_asm[r];
    const uint64_t first = (uint64_t)(tile - g.run_tile_off[r]) * SCR_TILE + (uint64_t)lane * SCR_L;
    const uint32_t n_mine = first < nk ? (uint32_t)(nk - first < SCR_L ? nk - first : SCR_L) : 0;
    const uint32_t k = g.k;
    const uint64_t mask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1;
    const uint32_t sh = 2 * (k - 1);
    unsigned long long hits = 0, atomics = 0;
    if (n_mine) {
        // the lane reads bases [pos, pos + k - 1 + n_mine), all inside the run
        uint64_t pos = g.run_base[r] + first, fwd = 0, rev = 0;
        uint32_t w = g.packed[pos >> 4] >> (2 * (uint32_t)(pos & 15)), left = 16 - (uint32_t)(pos & 15);
        auto roll = [&]() {
            if (left == 0) {
                w = g.packed[pos >> 4];
                left = 16;
            }
            const uint64_t c = w & 3u;
            w >>= 2;
            --left;
            ++pos;
            fwd = ((fwd << 2) | c) & mask;
            rev = (rev >> 2) | ((3 - c) << sh);
        };
        for (uint32_t i = 0; i + 1 < k; ++i) roll();
        uint64_t canon[SCR_L];
        uint32_t home[SCR_L], slot[SCR_L];
#pragma unroll
        for (uint32_t j = 0; j < SCR_L; ++j) {
            canon[j] = 0;
            if (j < n_mine) {
                roll();
                canon[j] = fwd < rev ? fwd : rev;
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
};

namespace sw {
namespace {

// kern(base, end, args ...) over [0, n) in launches of at most scr_launch_blocks() workgroups
template <class K, class... A> void launch_1d(K kern, uint64_t n, hipStream_t stream, A... args)
{
    const uint64_t per = (uint64_t)scr_launch_blocks() * SCR_TPB;
    for (uint64_t base = 0; base < n; base += per) {
        const uint64_t cnt = std::min<uint64_t>(per, n - base);
        hipLaunchKernelGGL(kern, dim3((unsigned)((cnt + SCR_TPB - 1) / SCR_TPB)), dim3(SCR_TPB), 0, stream, base, base + cnt, args...);
        SW_HIP(hipGetLastError());
    }
}

// at[i] = flagged elements before i, for i in [0, n]; returns at[n].  Synchronises the stream.
uint32_t scan_flags(const uint8_t *flag, uint32_t *at, uint64_t n, hipStream_t stream)
{
    size_t tmp_bytes = 0;
    auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), FlagAt{flag, n});
    SW_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, in, at, uint32_t(0), n + 1, rocprim::plus<uint32_t>(), stream));
    DevArray<unsigned char> tmp(tmp_bytes);
    SW_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, in, at, uint32_t(0), n + 1, rocprim::plus<uint32_t>(), stream));
    uint32_t total = 0;
    SW_HIP(hipMemcpyAsync(&total, at + n, 4, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    return total;
}

// n keys ascending in `keys` (which may end up pointing at `alt`'s block)
void sort_all_bits(uint64_t *&keys, uint64_t *&alt, uint64_t n, hipStream_t stream)
{
    if (n < 2) return;
    DevArray<uint32_t> d_fail(1);
    SW_HIP(hipMemsetAsync(d_fail.p, 0, 4, stream));
    sort_keys64(keys, alt, n, 0, 64, stream, d_fail.p);
    uint32_t failed = 0;
    SW_HIP(hipMemcpyAsync(&failed, d_fail.p, 4, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    check_sort_failed(failed);
}

void check_table_fail(const uint32_t *d_fail, hipStream_t stream)
{
    uint32_t f = 0;
    SW_HIP(hipMemcpyAsync(&f, d_fail, 4, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    if (f) raise(SW_ERR_RUNTIME, "internal error: the screen's k-mer table lost a key (%u)", f);
}

void batch_screen(const sw_batch &b, const uint64_t *offsets, const char *blob, uint64_t nq, uint32_t k, hipStream_t stream, sw_screen &o)
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

    // ---- query side: distinct canonical words, the table, numbers by first appearance, (word, mask) pairs per query ----
    uint64_t n_valid = 0, n_distinct = 0, cap = 0, n_pairs = 0;
    uint32_t bits = 0, chain = 0;
    DevArray<uint32_t> slots, pword, pmask;
    DevArray<uint64_t> by_number, pair_off(nq + 1);
    std::vector<uint64_t> pair_off_host(nq + 1, 0);
    if (text_bytes) {
        DevArray<uint8_t> text(text_bytes), flag(text_bytes);
        DevArray<uint64_t> d_off(nq + 1), word(text_bytes);
        DevArray<uint32_t> at(text_bytes + 1);
        up(text.p, blob, text_bytes);
        up(d_off.p, offsets, (nq + 1) * 8);
        launch_1d(k_scr_qwords, text_bytes, stream, (const uint8_t *)text.p, (const uint64_t *)d_off.p, (uint32_t)nq, k, word.p, flag.p);
        n_valid = scan_flags(flag.p, at.p, text_bytes, stream);
        if (n_valid) {
            DevArray<uint64_t> vword(n_valid), s_a(n_valid), s_b(n_valid), sorted_distinct;
            DevArray<uint32_t> vpos(n_valid), sidx(n_valid), first, number, d_stat(2);
            launch_1d(k_scr_compact, text_bytes, stream, (const uint8_t *)flag.p, (const uint32_t *)at.p, (const uint64_t *)word.p, vword.p, vpos.p);
            SW_HIP(hipMemcpyAsync(s_a.p, vword.p, n_valid * 8, hipMemcpyDeviceToDevice, stream));
            uint64_t *kp = s_a.p, *ap = s_b.p;
            sort_all_bits(kp, ap, n_valid, stream);
            launch_1d(k_scr_heads, n_valid, stream, (const uint64_t *)kp, 0u, flag.p);
            n_distinct = scan_flags(flag.p, at.p, n_valid, stream);
            if (n_distinct >= SCR_MAX_DISTINCT)
                raise(SW_ERR_VALUE, "screen: %llu distinct query k-mers; fewer than 2^31 are taken", (unsigned long long)n_distinct);
            sorted_distinct.alloc(n_distinct);
            launch_1d(k_scr_compact, n_valid, stream, (const uint8_t *)flag.p, (const uint32_t *)at.p, (const uint64_t *)kp, sorted_distinct.p, (uint32_t *)nullptr);
            // capacity: the power of two >= 2 |D| (the factor 2 has no measurement behind it); SEQWIN_AMD_SCR_TABLE_BITS (test library) sets it
            while ((1ull << bits) < 2 * n_distinct) ++bits;
            if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_SCR_TABLE_BITS")) {
                const uint64_t want = scr_env_u64(e, bits);
                if (want > 32 || (1ull << want) <= n_distinct)
                    raise(SW_ERR_VALUE, "screen: a table of 2^%llu slots does not exceed the %llu distinct query k-mers", (unsigned long long)want,
                          (unsigned long long)n_distinct);
                bits = (uint32_t)want;
            }
            cap = 1ull << bits;
            slots.alloc(cap);
            first.alloc(n_distinct);
            number.alloc(n_distinct);
            by_number.alloc(n_distinct);
            SW_HIP(hipMemsetAsync(slots.p, 0, cap * 4, stream));
            SW_HIP(hipMemsetAsync(first.p, 0xFF, n_distinct * 4, stream));
            SW_HIP(hipMemsetAsync(d_stat.p, 0, 8, stream));
            launch_1d(k_scr_insert, n_distinct, stream, (const uint64_t *)sorted_distinct.p, slots.p, cap, bits, d_stat.p, d_stat.p + 1);
            const Table by_sorted{slots.p, sorted_distinct.p, cap, bits};
            launch_1d(k_scr_first, n_valid, stream, by_sorted, (const uint64_t *)vword.p, sidx.p, first.p, d_stat.p + 1);
            check_table_fail(d_stat.p + 1, stream);
            launch_1d(k_scr_is_first, n_valid, stream, (const uint32_t *)sidx.p, (const uint32_t *)first.p, flag.p);
            const uint64_t numbered = scan_flags(flag.p, at.p, n_valid, stream);
            if (numbered != n_distinct)
                raise(SW_ERR_RUNTIME, "internal error: %llu of %llu distinct query k-mers were numbered", (unsigned long long)numbered, (unsigned long long)n_distinct);
            launch_1d(k_scr_number, n_valid, stream, (const uint8_t *)flag.p, (const uint32_t *)at.p, (const uint32_t *)sidx.p, (const uint64_t *)vword.p, number.p,
                      by_number.p);
            launch_1d(k_scr_relabel, cap, stream, slots.p, (const uint32_t *)number.p);
            SW_HIP(hipMemcpyAsync(&chain, d_stat.p, 4, hipMemcpyDeviceToHost, stream));
            // pairs: (query << 32 | number) ascending; a run of equal (query, number >> 5) is one pair
            launch_1d(k_scr_qkeys, n_valid, stream, (const uint32_t *)vpos.p, (const uint32_t *)sidx.p, (const uint32_t *)number.p, (const uint64_t *)d_off.p,
                      (uint32_t)nq, s_a.p);
            kp = s_a.p;
            ap = s_b.p;
            sort_all_bits(kp, ap, n_valid, stream);
            launch_1d(k_scr_heads, n_valid, stream, (const uint64_t *)kp, 5u, flag.p);
            n_pairs = scan_flags(flag.p, at.p, n_valid, stream);
            pword.alloc(n_pairs);
            pmask.alloc(n_pairs);
            DevArray<uint32_t> d_np(nq), d_nk(nq);
            SW_HIP(hipMemsetAsync(pmask.p, 0, n_pairs * 4, stream));
            SW_HIP(hipMemsetAsync(d_np.p, 0, nq * 4, stream));
            SW_HIP(hipMemsetAsync(d_nk.p, 0, nq * 4, stream));
            launch_1d(k_scr_pairs, n_valid, stream, (const uint64_t *)kp, (const uint8_t *)flag.p, (const uint32_t *)at.p, pword.p, pmask.p, d_np.p, d_nk.p);
            std::vector<uint32_t> np(nq);
            SW_HIP(hipMemcpyAsync(np.data(), d_np.p, nq * 4, hipMemcpyDeviceToHost, stream));
            SW_HIP(hipMemcpyAsync(o.n_kmers.data(), d_nk.p, nq * 4, hipMemcpyDeviceToHost, stream));
            SW_HIP(hipStreamSynchronize(stream));
            for (uint64_t q = 0; q < nq; ++q) pair_off_host[q + 1] = pair_off_host[q] + np[q];
            if (pair_off_host[nq] != n_pairs) raise(SW_ERR_RUNTIME, "internal error: the queries' pair lists do not add up");
        }
    }
    up(pair_off.p, pair_off_host.data(), (nq + 1) * 8);
    o.n_distinct = n_distinct;
    SW_HIP(hipEventRecord(e1, stream));

    // ---- the valid runs of length >= k, once per call (as sw_batch_minhash takes them) ----
    std::vector<uint64_t> run_base;
    std::vector<uint32_t> run_nk, run_asm, run_tile_off, asm_tile_off(n_asm + 1, 0);
    std::vector<uint64_t> asm_kmers(n_asm + 1, 0);   // k-mers of the assemblies before a
    uint64_t tiles = 0;
    for (uint64_t a = 0; a < n_asm; ++a) {
        asm_tile_off[a] = (uint32_t)tiles;
        asm_kmers[a + 1] = asm_kmers[a];
        for (uint32_t r = h.record_offsets[a]; r < h.record_offsets[a + 1]; ++r)
            for (uint32_t q = h.rec_run_off[r]; q < h.rec_run_off[r + 1]; ++q) {
                if (h.run_len[q] < k) continue;
                const uint32_t nk = h.run_len[q] - k + 1;
                run_base.push_back(h.rec_base[r] + h.run_pos[q]);
                run_nk.push_back(nk);
                run_asm.push_back((uint32_t)a);
                run_tile_off.push_back((uint32_t)tiles);
                tiles += ((uint64_t)nk + SCR_TILE - 1) / SCR_TILE;
                asm_kmers[a + 1] += nk;
                if (tiles >= 0xFFFFFFFFull) raise(SW_ERR_RUNTIME, "screen: the batch has more k-mers than one call takes (2^32 tiles of %u)", SCR_TILE);
            }
    }
    asm_tile_off[n_asm] = (uint32_t)tiles;
    run_tile_off.push_back((uint32_t)tiles);
    const uint64_t n_runs = run_nk.size();
    if (n_runs >= 0xFFFFFFFFull) raise(SW_ERR_RUNTIME, "screen: %llu valid runs exceed 32-bit indices", (unsigned long long)n_runs);

    // ---- probe and reduce, a chunk of assemblies at a time ----
    uint64_t probed = 0, launches = 0, chunks = 0;
    unsigned long long stat[2] = {};
    std::vector<std::unique_ptr<Event>> ev;
    if (n_distinct && n_asm && nq) {
        const uint64_t words = (n_distinct + 31) / 32;
        // the bitmap's budget changes speed only; 1 GiB has no measurement behind it.  SEQWIN_AMD_SCR_BITMAP_KB (test library) sets it
        uint64_t budget = SCR_BITMAP_BYTES;
        if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_SCR_BITMAP_KB")) budget = scr_env_u64(e, budget >> 10) << 10;
        const uint64_t rows_max = std::min<uint64_t>(std::max<uint64_t>(budget / (words * 4), 1), n_asm);
        DevArray<uint32_t> bitmap(rows_max * words);
        DevArray<uint64_t> d_run_base(n_runs);
        DevArray<uint32_t> d_run_nk(n_runs), d_run_asm(n_runs), d_run_tile(n_runs + 1);
        DevArray<unsigned long long> d_stat(2);
        up(d_run_base.p, run_base.data(), n_runs * 8);
        up(d_run_nk.p, run_nk.data(), n_runs * 4);
        up(d_run_asm.p, run_asm.data(), n_runs * 4);
        up(d_run_tile.p, run_tile_off.data(), (n_runs + 1) * 4);
        SW_HIP(hipMemsetAsync(d_stat.p, 0, 16, stream));
        SW_HIP(hipMemsetAsync(bitmap.p, 0, rows_max * words * 4, stream));
        ProbeArgs g{};
        g.packed = b.d_packed.p;
        g.run_base = d_run_base.p;
        g.run_nk = d_run_nk.p;
        g.run_asm = d_run_asm.p;
        g.run_tile_off = d_run_tile.p;
        g.n_runs = (uint32_t)n_runs;
        g.t = Table{slots.p, by_number.p, cap, bits};
        g.bitmap = bitmap.p;
        g.words = words;
        g.stat = d_stat.p;
        g.k = k;
        const uint64_t blocks_max = scr_launch_blocks(), tile_step = blocks_max * SCR_WPB;
        const uint32_t q_step = (uint32_t)std::max<uint64_t>(blocks_max / ((rows_max + SCR_RED_ROWS - 1) / SCR_RED_ROWS), 1);
        for (uint64_t a0 = 0; a0 < n_asm; a0 += rows_max, ++chunks) {
            const uint64_t a1 = std::min<uint64_t>(n_asm, a0 + rows_max), rows = a1 - a0;
            for (int i = 0; i < 3; ++i) ev.emplace_back(new Event);
            SW_HIP(hipEventRecord(*ev[3 * chunks], stream));
            g.asm0 = (uint32_t)a0;
            for (uint64_t t0 = asm_tile_off[a0]; t0 < asm_tile_off[a1]; t0 += tile_step, ++launches) {
                g.tile_begin = (uint32_t)t0;
                g.tile_end = (uint32_t)std::min<uint64_t>(asm_tile_off[a1], t0 + tile_step);
                const uint64_t n_tiles = (uint64_t)g.tile_end - g.tile_begin;
                hipLaunchKernelGGL(k_scr_probe, dim3((unsigned)((n_tiles + SCR_WPB - 1) / SCR_WPB)), dim3(SCR_TPB), 0, stream, g);
                SW_HIP(hipGetLastError());
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
            if (a1 < n_asm) SW_HIP(hipMemsetAsync(bitmap.p, 0, rows * words * 4, stream));   // (cleared for the next chunk)
            SW_HIP(hipEventRecord(*ev[3 * chunks + 2], stream));
        }
        SW_HIP(hipMemcpyAsync(stat, d_stat.p, 16, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));   // (the temporaries go back to the pool behind the kernels)
    }
    SW_HIP(hipStreamSynchronize(stream));
    float ms = 0;
    SW_HIP(hipEventElapsedTime(&ms, e0, e1));
    o.ms[0] = ms;
    for (uint64_t c = 0; c < chunks; ++c) {
        SW_HIP(hipEventElapsedTime(&ms, *ev[3 * c], *ev[3 * c + 1]));
        o.chunk_probe_ms.push_back(ms);
        o.ms[1] += ms;
        SW_HIP(hipEventElapsedTime(&ms, *ev[3 * c + 1], *ev[3 * c + 2]));
        o.chunk_reduce_ms.push_back(ms);
        o.ms[2] += ms;
    }
    const uint64_t cn[10] = {text_bytes, n_valid, n_distinct, cap, chain, probed, stat[0], stat[1], chunks, launches};
    memcpy(o.counters, cn, sizeof cn);
}

}  // namespace
}  // namespace sw

using namespace sw;

extern "C" {

int sw_batch_screen(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, void *stream, sw_screen **out)
{
    return guarded([&] {
        if (k < 1 || k > 32) raise(SW_ERR_VALUE, "screen: k-mer length must lie in 1..32 (got %llu)", (unsigned long long)k);
        if (!batch || !out || (n_queries && !offsets)) raise(SW_ERR_VALUE, "screen: a NULL handle or array");
        if (n_queries >= 0xFFFFFFFFull) raise(SW_ERR_VALUE, "screen: %llu queries exceed 32-bit indices", (unsigned long long)n_queries);
        if (n_queries) {
            if (offsets[0] != 0) raise(SW_ERR_VALUE, "screen: offsets must start at 0");
            for (uint64_t q = 0; q < n_queries; ++q)
                if (offsets[q] > offsets[q + 1]) raise(SW_ERR_VALUE, "screen: offsets must be non-decreasing (query %llu)", (unsigned long long)q);
            if (offsets[n_queries] >= SCR_MAX_TEXT)
                raise(SW_ERR_VALUE, "screen: %llu bytes of query text; fewer than 2^32 - 256 are taken", (unsigned long long)offsets[n_queries]);
            if (offsets[n_queries] && !blob) raise(SW_ERR_VALUE, "screen: a NULL handle or array");
        }
        scr_require_device(batch->device, "the batch");
        StreamScope scope((hipStream_t)stream);
        std::unique_ptr<sw_screen> o(new sw_screen);
        o->device = batch->device;
        batch_screen(*batch, offsets, blob, n_queries, (uint32_t)k, (hipStream_t)stream, *o);
        *out = o.release();
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
        if (r0 > r1 || r1 > h->nq || c0 > c1 || c1 > h->n_asm)
            raise(SW_ERR_VALUE, "screen: rows [%llu, %llu) x columns [%llu, %llu) lie outside the %llu queries x %llu assemblies", (unsigned long long)r0,
                  (unsigned long long)r1, (unsigned long long)c0, (unsigned long long)c1, (unsigned long long)h->nq, (unsigned long long)h->n_asm);
        const uint64_t nr = r1 - r0, nc = c1 - c0;
        if (!nr || !nc) return;
        if (!counts) raise(SW_ERR_VALUE, "screen: a NULL handle or array");
        scr_require_device(h->device, "the screen");
        SW_HIP(hipMemcpy2D(counts, nc * 4, h->counts.p + r0 * h->n_asm + c0, h->n_asm * 4, nc * 4, nr, hipMemcpyDeviceToHost));
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
