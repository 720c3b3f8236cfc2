// screen_core.hpp -- the query side of screen.hip, shared with hits.hip: the check of the caller's queries, the canonical words of the
// query text, the distinct words, the open-addressing table over them and their numbers by first appearance.  The batch side -- the
// valid runs cut into tiles, the walk of the probe kernels of both files -- is kmer_walk.hpp.  Device functions cannot be linked
// across translation units here, so both files include this header.
#pragma once
#include <cstring>  // rocprim's texture iterator needs ::memset declared first
#include <memory>

#include <rocprim/rocprim.hpp>

#include "kmer_walk.hpp"

namespace sw {
namespace {

constexpr uint32_t SCR_TPB = KW_TPB, SCR_WAVE = KW_WAVE, SCR_WPB = KW_WPB, SCR_L = KW_L, SCR_MAX_BLOCKS = KW_MAX_BLOCKS;   // (kmer_walk.hpp)
constexpr uint64_t SCR_MAX_TEXT = 0xFFFFFFFFull - 255; // query text: fewer bytes than this (a thread per byte in workgroups of 256)
constexpr uint64_t SCR_MAX_DISTINCT = 1ull << 31;     // distinct query k-mers: fewer than this (a slot holds number + 1 in 32 bits)
constexpr uint64_t SCR_BITMAP_BYTES = 1ull << 30;     // budget of the presence bitmap: speed only, chosen without a measurement
constexpr uint32_t SCR_RED_ROWS = 64;                 // assemblies per workgroup of k_scr_reduce (16 per wave)
constexpr uint32_t SCR_NONE = 0xFFFFFFFFu;

// workgroups per launch of the query side's kernels: launch_blocks(SCR_BLOCKS_ENV); the switch (test library) lowers it so that a
// small input needs several launches
constexpr const char *SCR_BLOCKS_ENV = "SEQWIN_AMD_SCR_MAX_BLOCKS";

// what a call says about its queries by itself; what: the caller's name in the messages
void check_queries(const char *what, const uint64_t *offsets, const char *blob, uint64_t nq)
{
    if (nq && !offsets) raise(SW_ERR_VALUE, "%s: a NULL handle or array", what);
    if (nq >= 0xFFFFFFFFull) raise(SW_ERR_VALUE, "%s: %llu queries exceed 32-bit indices", what, (unsigned long long)nq);
    if (!nq) return;
    if (offsets[0] != 0) raise(SW_ERR_VALUE, "%s: offsets must start at 0", what);
    for (uint64_t q = 0; q < nq; ++q)
        if (offsets[q] > offsets[q + 1]) raise(SW_ERR_VALUE, "%s: offsets must be non-decreasing (query %llu)", what, (unsigned long long)q);
    if (offsets[nq] >= SCR_MAX_TEXT) raise(SW_ERR_VALUE, "%s: %llu bytes of query text; fewer than 2^32 - 256 are taken", what, (unsigned long long)offsets[nq]);
    if (offsets[nq] && !blob) raise(SW_ERR_VALUE, "%s: a NULL handle or array", what);
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

// kern(base, end, args ...) over [0, n) in launches of at most launch_blocks(SCR_BLOCKS_ENV) workgroups
template <class K, class... A> void launch_1d(K kern, uint64_t n, hipStream_t stream, A... args)
{
    const uint64_t per = (uint64_t)launch_blocks(SCR_BLOCKS_ENV) * SCR_TPB;
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

// ---- the query side as one object ---------------------------------------------------------------------------------------------
// What batch_screen and batch_best_hits build first.  slots / by_number are the table the probe kernels read (a slot holds
// number + 1, by_number[number] = the word); the rest is what made it, kept until release_temporaries() for a caller that derives
// more from it (hits.hip: multiplicities and the seed table).
struct QuerySide {
    uint64_t text_bytes = 0, n_valid = 0, n_distinct = 0, cap = 0;
    uint32_t bits = 0, chain = 0;
    DevArray<uint32_t> slots;
    DevArray<uint64_t> by_number;
    // temporaries
    DevArray<uint8_t> text, flag;      // [text_bytes]
    DevArray<uint64_t> d_off, word;    // [nq + 1], [text_bytes]
    DevArray<uint32_t> at;             // [text_bytes + 1]
    DevArray<uint64_t> vword, s_a, s_b, sorted_distinct;   // [n_valid] ..., [n_distinct]
    DevArray<uint32_t> vpos, sidx, first, number, d_stat;  // [n_valid] the text position and the sorted index of every valid word; [n_distinct]
    Table table() const { return Table{slots.p, by_number.p, cap, bits}; }
    void release_temporaries()
    {
        text.release(); flag.release(); d_off.release(); word.release(); at.release();
        vword.release(); s_a.release(); s_b.release(); sorted_distinct.release();
        vpos.release(); sidx.release(); first.release(); number.release(); d_stat.release();
    }
};

// distinct canonical words of the query text, the table over them, numbers by first appearance.  Leaves the stream synchronised.
void build_query_side(const uint64_t *offsets, const char *blob, uint64_t nq, uint32_t k, hipStream_t stream, QuerySide &Q)
{
    Q.text_bytes = nq ? offsets[nq] : 0;
    const uint64_t text_bytes = Q.text_bytes;
    if (!text_bytes) return;
    Q.text.alloc(text_bytes);
    Q.flag.alloc(text_bytes);
    Q.d_off.alloc(nq + 1);
    Q.word.alloc(text_bytes);
    Q.at.alloc(text_bytes + 1);
    SW_HIP(hipMemcpyAsync(Q.text.p, blob, text_bytes, hipMemcpyHostToDevice, stream));
    SW_HIP(hipMemcpyAsync(Q.d_off.p, offsets, (nq + 1) * 8, hipMemcpyHostToDevice, stream));
    launch_1d(k_scr_qwords, text_bytes, stream, (const uint8_t *)Q.text.p, (const uint64_t *)Q.d_off.p, (uint32_t)nq, k, Q.word.p, Q.flag.p);
    const uint64_t n_valid = Q.n_valid = scan_flags(Q.flag.p, Q.at.p, text_bytes, stream);
    if (!n_valid) return;
    Q.vword.alloc(n_valid);
    Q.s_a.alloc(n_valid);
    Q.s_b.alloc(n_valid);
    Q.vpos.alloc(n_valid);
    Q.sidx.alloc(n_valid);
    Q.d_stat.alloc(2);
    launch_1d(k_scr_compact, text_bytes, stream, (const uint8_t *)Q.flag.p, (const uint32_t *)Q.at.p, (const uint64_t *)Q.word.p, Q.vword.p, Q.vpos.p);
    SW_HIP(hipMemcpyAsync(Q.s_a.p, Q.vword.p, n_valid * 8, hipMemcpyDeviceToDevice, stream));
    uint64_t *kp = Q.s_a.p, *ap = Q.s_b.p;
    sort_all_bits(kp, ap, n_valid, stream);
    launch_1d(k_scr_heads, n_valid, stream, (const uint64_t *)kp, 0u, Q.flag.p);
    const uint64_t n_distinct = Q.n_distinct = scan_flags(Q.flag.p, Q.at.p, n_valid, stream);
    if (n_distinct >= SCR_MAX_DISTINCT)
        raise(SW_ERR_VALUE, "screen: %llu distinct query k-mers; fewer than 2^31 are taken", (unsigned long long)n_distinct);
    Q.sorted_distinct.alloc(n_distinct);
    launch_1d(k_scr_compact, n_valid, stream, (const uint8_t *)Q.flag.p, (const uint32_t *)Q.at.p, (const uint64_t *)kp, Q.sorted_distinct.p, (uint32_t *)nullptr);
    // capacity: the power of two >= 2 |D| (the factor 2 has no measurement behind it); SEQWIN_AMD_SCR_TABLE_BITS (test library) sets it
    uint32_t bits = 0;
    while ((1ull << bits) < 2 * n_distinct) ++bits;
    if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_SCR_TABLE_BITS")) {
        const uint64_t want = env_u64(e, bits);
        if (want > 32 || (1ull << want) <= n_distinct)
            raise(SW_ERR_VALUE, "screen: a table of 2^%llu slots does not exceed the %llu distinct query k-mers", (unsigned long long)want,
                  (unsigned long long)n_distinct);
        bits = (uint32_t)want;
    }
    Q.bits = bits;
    const uint64_t cap = Q.cap = 1ull << bits;
    Q.slots.alloc(cap);
    Q.first.alloc(n_distinct);
    Q.number.alloc(n_distinct);
    Q.by_number.alloc(n_distinct);
    SW_HIP(hipMemsetAsync(Q.slots.p, 0, cap * 4, stream));
    SW_HIP(hipMemsetAsync(Q.first.p, 0xFF, n_distinct * 4, stream));
    SW_HIP(hipMemsetAsync(Q.d_stat.p, 0, 8, stream));
    launch_1d(k_scr_insert, n_distinct, stream, (const uint64_t *)Q.sorted_distinct.p, Q.slots.p, cap, bits, Q.d_stat.p, Q.d_stat.p + 1);
    const Table by_sorted{Q.slots.p, Q.sorted_distinct.p, cap, bits};
    launch_1d(k_scr_first, n_valid, stream, by_sorted, (const uint64_t *)Q.vword.p, Q.sidx.p, Q.first.p, Q.d_stat.p + 1);
    check_table_fail(Q.d_stat.p + 1, stream);
    launch_1d(k_scr_is_first, n_valid, stream, (const uint32_t *)Q.sidx.p, (const uint32_t *)Q.first.p, Q.flag.p);
    const uint64_t numbered = scan_flags(Q.flag.p, Q.at.p, n_valid, stream);
    if (numbered != n_distinct)
        raise(SW_ERR_RUNTIME, "internal error: %llu of %llu distinct query k-mers were numbered", (unsigned long long)numbered, (unsigned long long)n_distinct);
    launch_1d(k_scr_number, n_valid, stream, (const uint8_t *)Q.flag.p, (const uint32_t *)Q.at.p, (const uint32_t *)Q.sidx.p, (const uint64_t *)Q.vword.p, Q.number.p,
              Q.by_number.p);
    launch_1d(k_scr_relabel, cap, stream, Q.slots.p, (const uint32_t *)Q.number.p);
    SW_HIP(hipMemcpyAsync(&Q.chain, Q.d_stat.p, 4, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
}

}  // namespace
}  // namespace sw
