// minhash.hip -- Mash-compatible MinHash sketches of a resident batch and pairwise Jaccard counts on the device.
//
// Replaces Assemblies.mash (src/seqwin/assemblies.py:76-99: `mash sketch` over every assembly, `mash dist` over all pairs, the
// output parsed as text) and the two reductions kmers.filter_graph takes from its matrix (src/seqwin/kmers.py:315-323, 419-420).
// The specification followed is Mash 2.x at its defaults, as DESIGN.md section 3 states it; tests/tools/minhash_host.py is its
// host restatement.  Agreement with the `mash` binary itself has never been observed.
//
//   k_mh_hash     one pass over the packed words by the batch's run / tile / lane walk (kmer_walk.hpp): a lane holds MH_L consecutive
//                 k-mers of one valid run, expands the canonical one of every pair of rolled words to its ASCII bytes and runs
//                 MurmurHash3_x64_128 on them; hashes at or below the assembly's threshold are appended to its candidate range
//                 (one atomic per wave)
//   k_mh_select   one workgroup per assembly: bitonic sort of the candidates in LDS, duplicates dropped, the S smallest kept
//   general route an assembly that fell short (fewer than S distinct candidates under a threshold below the whole range, or more
//                 candidates than the range holds) is finished exactly, once: all its k-mers hashed into a scratch, sorted by the
//                 library's keys-only radix sort, the first S distinct values taken
//   k_mh_pairs    a block of rows against a block of columns: the row's sketch in LDS, a wave per column sketch, every lane ranks
//                 its element in the row by binary search
//   k_mh_rowsum   sum over a row of 2J / (1 + J) in f64, in a fixed order
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>

#include "kmer_walk.hpp"

namespace sw {
namespace {

constexpr uint32_t MH_TPB = KW_TPB, MH_WAVE = KW_WAVE, MH_TILE = KW_TILE, MH_MAX_BLOCKS = KW_MAX_BLOCKS;   // (kmer_walk.hpp)
constexpr uint32_t MH_SEL_MAX = 16384;              // most candidates a workgroup sorts in LDS (128 KiB of 64-bit values)
constexpr uint32_t MH_PAIR_COLS = 64;               // column sketches per workgroup of k_mh_pairs (16 per wave)
constexpr uint32_t MH_PAIR_LDS_BYTES = 48 * 1024;   // a longer row sketch is searched in global memory
constexpr uint64_t MM_C1 = 0x87c37b91114253d5ULL, MM_C2 = 0x4cf5ad432745937fULL;

// workgroups per launch of the hash pass and of the pair kernel: launch_blocks(MH_BLOCKS_ENV); the switch (test library) lowers it
constexpr const char *MH_BLOCKS_ENV = "SEQWIN_AMD_MH_MAX_BLOCKS";

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

__device__ __forceinline__ uint64_t fmix64(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// four 2-bit codes (bits 0..7, the first base lowest) -> their four ASCII letters, the first base in the low byte:
// 'A' + {0, 2, 6, 19} = A C G T
__device__ __forceinline__ uint32_t ascii4(uint32_t x)
{
    uint32_t t = (x | (x << 12)) & 0x000F000Fu;
    t = (t | (t << 6)) & 0x03030303u;
    const uint32_t lo = t & 0x01010101u, hi = (t >> 1) & 0x01010101u, both = lo & hi;
    return 0x41414141u + (lo << 1) + hi * 6u + both * 11u;
}

// bytes 8m .. 8m + 7 of the k-mer whose codes lie in cl with the FIRST base lowest; m <= 3
__device__ __forceinline__ uint64_t ascii_word(uint64_t cl, uint32_t m)
{
    const uint32_t x = (uint32_t)(cl >> (16 * m)) & 0xFFFFu;
    return (uint64_t)ascii4(x & 0xFFu) | ((uint64_t)ascii4(x >> 8) << 32);
}

// h1 of MurmurHash3_x64_128 over the k ASCII bytes; NB = k / 16 whole blocks, the tail's byte masks m1 / m2 are uniform
template <int NB> __device__ __forceinline__ uint64_t mm3_h1(uint64_t cl, uint32_t k, uint32_t seed, uint64_t m1, uint64_t m2)
{
    uint64_t h1 = seed, h2 = seed;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        uint64_t k1 = ascii_word(cl, 2 * b), k2 = ascii_word(cl, 2 * b + 1);
        k1 *= MM_C1; k1 = rotl64(k1, 31); k1 *= MM_C2; h1 ^= k1;
        h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        k2 *= MM_C2; k2 = rotl64(k2, 33); k2 *= MM_C1; h2 ^= k2;
        h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    }
    if (NB < 2) {   // (k = 32 is two blocks and no tail)
        const uint32_t tl = k & 15u;
        if (tl > 8) {
            uint64_t k2 = ascii_word(cl, 2 * NB + 1) & m2;
            k2 *= MM_C2; k2 = rotl64(k2, 33); k2 *= MM_C1; h2 ^= k2;
        }
        if (tl > 0) {
            uint64_t k1 = ascii_word(cl, 2 * NB) & m1;
            k1 *= MM_C1; k1 = rotl64(k1, 31); k1 *= MM_C2; h1 ^= k1;
        }
    }
    h1 ^= k; h2 ^= k;
    h1 += h2; h2 += h1;
    h1 = fmix64(h1); h2 = fmix64(h2);
    return h1 + h2;
}

struct HashArgs {
    RunView v;
    const uint64_t *thr;             // [n_asm] a hash <= thr[a] is a candidate (single: every hash is)
    unsigned long long *cnt;         // [n_asm] candidates seen (single: one counter)
    uint64_t *cand;                  // assembly a's range: cand[a * cap, (a + 1) * cap) (single: cand[0, cap))
    uint64_t cap;
    uint32_t single;                 // 1: the general route of one assembly
    uint32_t k, seed, bits32;
    uint64_t m1, m2;                 // byte masks of the tail's two words
};

template <int NB> __global__ __launch_bounds__(MH_TPB) void k_mh_hash(HashArgs g)
{
    __shared__ uint64_t stash[MH_TPB / MH_WAVE][MH_TILE];   // a lane's i-th candidate at [i * 64 + lane]
    const uint32_t wave = threadIdx.x / MH_WAVE, lane = threadIdx.x % MH_WAVE;
    uint32_t r, n_mine;
    uint64_t first;
    if (!wave_tile(g.v, lane, r, first, n_mine)) return;   // (the whole wave)
    const uint32_t a = g.v.run_asm[r];
    const uint64_t T = g.single ? ~0ull : g.thr[a];
    const uint32_t k = g.k;
    uint32_t n_out = 0;
    KmerRoller R(g.v.packed, k);
    if (n_mine) {
        R.start(g.v.run_base[r] + first);
        const uint32_t nb = k - 1 + n_mine;
        for (uint32_t i = 0; i < nb; ++i) {
            R.roll();
            if (i + 1 >= k) {
                // the canonical k-mer with its first base LOWEST is the complement of the other strand's word
                const uint64_t cl = ~(R.fwd > R.rev ? R.fwd : R.rev) & R.mask;
                uint64_t h = mm3_h1<NB>(cl, k, g.seed, g.m1, g.m2);
                if (g.bits32) h &= 0xFFFFFFFFull;
                if (h <= T) {
                    stash[wave][n_out * MH_WAVE + lane] = h;
                    ++n_out;
                }
            }
        }
    }
    const WaveRange w = wave_append(g.cnt + (g.single ? 0 : a), lane, n_out);   // one atomic per wave
    if (w.total == 0) return;
    const uint64_t at = w.base + w.offset;
    uint64_t *dst = g.cand + (g.single ? 0 : (uint64_t)a * g.cap);
    for (uint32_t i = 0; i < n_out; ++i)
        if (at + i < g.cap) dst[at + i] = stash[wave][i * MH_WAVE + lane];   // a count beyond the capacity is recorded, not written
}

// One workgroup per assembly: its candidates sorted in LDS, duplicates dropped, the S smallest written to tmp[ub_off[a] ...].
// fall[a] = 1: the assembly goes through the general route.
__global__ __launch_bounds__(MH_TPB) void k_mh_select(const uint64_t *__restrict__ cand, const unsigned long long *__restrict__ cnt, uint64_t cap,
                                                      const uint8_t *__restrict__ whole, uint64_t S, const uint64_t *__restrict__ ub_off,
                                                      uint64_t *__restrict__ tmp, uint32_t *__restrict__ sk_len, uint8_t *__restrict__ fall)
{
    extern __shared__ uint64_t v[];   // the smallest power of two >= cap entries
    __shared__ uint32_t part[MH_TPB + 1];
    const uint32_t a = blockIdx.x, tid = threadIdx.x;
    const unsigned long long n64 = cnt[a];
    if (n64 > cap) {
        if (tid == 0) {
            fall[a] = 1;
            sk_len[a] = 0;
        }
        return;
    }
    const uint32_t n = (uint32_t)n64;
    uint32_t P = 1;
    while (P < n) P <<= 1;
    for (uint32_t i = tid; i < P; i += MH_TPB) v[i] = i < n ? cand[(uint64_t)a * cap + i] : ~0ull;   // (padding sorts last: only v[0, n) counts)
    __syncthreads();
    for (uint32_t kk = 2; kk <= P; kk <<= 1)
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < P; i += MH_TPB) {
                const uint32_t p = i ^ j;
                if (p > i) {
                    const uint64_t x = v[i], y = v[p];
                    if ((x > y) == ((i & kk) == 0)) {
                        v[i] = y;
                        v[p] = x;
                    }
                }
            }
            __syncthreads();
        }
    const uint32_t chunk = (n + MH_TPB - 1) / MH_TPB, b = tid * chunk < n ? tid * chunk : n, e = b + chunk < n ? b + chunk : n;
    uint32_t heads = 0;
    for (uint32_t i = b; i < e; ++i) heads += (i == 0 || v[i] != v[i - 1]) ? 1u : 0u;
    part[tid] = heads;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < MH_TPB; ++t) {
            const uint32_t x = part[t];
            part[t] = run;
            run += x;
        }
        part[MH_TPB] = run;
    }
    __syncthreads();
    uint64_t rank = part[tid];
    uint64_t *out = tmp + ub_off[a];
    for (uint32_t i = b; i < e; ++i)
        if (i == 0 || v[i] != v[i - 1]) {
            if (rank < S) out[rank] = v[i];   // (rank < the assembly's distinct hashes <= its k-mers: inside its range)
            ++rank;
        }
    if (tid == 0) {
        const uint64_t d = part[MH_TPB];
        const bool done = d >= S || whole[a];
        fall[a] = done ? 0 : 1;
        sk_len[a] = done ? (uint32_t)(d < S ? d : S) : 0u;
    }
}

// The first S distinct values of n ascending keys (one workgroup walks them in order)
__global__ __launch_bounds__(MH_TPB) void k_mh_take(const uint64_t *__restrict__ v, uint64_t n, uint64_t S, uint64_t *__restrict__ out,
                                                    uint32_t *__restrict__ len)
{
    __shared__ uint32_t wtot[MH_TPB / MH_WAVE];
    const uint32_t tid = threadIdx.x, wave = tid / MH_WAVE, lane = tid % MH_WAVE;
    uint64_t count = 0;   // (uniform)
    for (uint64_t base = 0; base < n && count < S; base += MH_TPB) {
        const uint64_t i = base + tid;
        const bool head = i < n && (i == 0 || v[i] != v[i - 1]);
        const unsigned long long m = __ballot(head);
        if (lane == 0) wtot[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t x = 0; x < MH_TPB / MH_WAVE; ++x) {
            if (x < wave) before += wtot[x];
            all += wtot[x];
        }
        const uint64_t rank = count + before + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (head && rank < S) out[rank] = v[i];
        count += all;
        __syncthreads();
    }
    if (tid == 0) *len = (uint32_t)(count < S ? count : S);
}

template <class T> __global__ void k_mh_compact(const uint64_t *__restrict__ tmp, const uint64_t *__restrict__ ub_off, const uint64_t *__restrict__ off,
                                               T *__restrict__ out)
{
    const uint32_t a = blockIdx.x;
    const uint64_t o = off[a], n = off[a + 1] - o, s = ub_off[a];
    for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) out[o + i] = (T)tmp[s + i];
}

// (shared, total) of rows [r0, r0 + n_rows) x columns [c0, c0 + n_cols) as `mash dist` counts them.  The walk of two ascending
// lists A and B visits the distinct values of their union in ascending order and stops after S of them or where a list runs out;
// every common value lies at or before that place.  So, with rank_U(x) = the number of union values <= x,
//     shared = #{ x in both : rank_U(x) <= S },   total = min(S, |A| + |B| - |both|),
// and rank_U(x) = (values of A <= x) + (values of B <= x) - (common values <= x): no lane walks, nothing depends on a split.
template <class T, bool IN_LDS>
__global__ __launch_bounds__(MH_TPB) void k_mh_pairs(const uint64_t *__restrict__ off, const T *__restrict__ hs, uint32_t r0, uint32_t c0,
                                                     uint32_t n_cols, uint32_t col_tiles, uint64_t S, uint32_t *__restrict__ shared,
                                                     uint32_t *__restrict__ total)
{
    extern __shared__ uint64_t mh_row_raw[];
    T *row_l = reinterpret_cast<T *>(mh_row_raw);
    const uint32_t tid = threadIdx.x, wave = tid / MH_WAVE, lane = tid % MH_WAVE;
    const uint32_t rl = blockIdx.x / col_tiles, ct = blockIdx.x % col_tiles;
    const uint64_t a0 = off[r0 + rl];
    const uint32_t na = (uint32_t)(off[r0 + rl + 1] - a0);
    const T *A = hs + a0;
    if (IN_LDS) {
        for (uint32_t i = tid; i < na; i += MH_TPB) row_l[i] = hs[a0 + i];
        __syncthreads();
        A = row_l;
    }
    const uint32_t c_end = (ct + 1) * MH_PAIR_COLS < n_cols ? (ct + 1) * MH_PAIR_COLS : n_cols;
    for (uint32_t cc = ct * MH_PAIR_COLS + wave; cc < c_end; cc += MH_TPB / MH_WAVE) {   // (uniform in the wave)
        const uint64_t b0 = off[c0 + cc];
        const uint32_t nb = (uint32_t)(off[c0 + cc + 1] - b0);
        uint32_t both = 0, sh = 0;
        for (uint32_t base = 0; base < nb; base += MH_WAVE) {
            const uint32_t j = base + lane;
            const bool act = j < nb;
            const T x = act ? hs[b0 + j] : (T)0;
            uint32_t lo = 0, hi = act ? na : 0;   // values of A below x
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (A[mid] < x) lo = mid + 1; else hi = mid;
            }
            const bool match = act && lo < na && A[lo] == x;
            const unsigned long long m = __ballot(match);
            const uint32_t c_incl = both + (uint32_t)__popcll(m & ((2ull << lane) - 1));   // common values <= x
            const bool in = match && (uint64_t)j + 1 + (uint64_t)lo + 1 - c_incl <= S;
            sh += (uint32_t)__popcll(__ballot(in));
            both += (uint32_t)__popcll(m);
        }
        if (lane == 0) {
            const uint64_t u = (uint64_t)na + nb - both, at = (uint64_t)rl * n_cols + cc;
            shared[at] = sh;
            total[at] = (uint32_t)(u < S ? u : S);
        }
    }
}

// rowsum[r] = sum over the row's columns of 2J / (1 + J), J = shared / total in f64: every thread adds its columns in
// ascending order, the 256 partial sums are added by a fixed tree.  zero: a pair with total == 0 was seen.
__global__ __launch_bounds__(MH_TPB) void k_mh_rowsum(const uint32_t *__restrict__ shared, const uint32_t *__restrict__ total, uint32_t n_cols,
                                                      double *__restrict__ rowsum, uint32_t *__restrict__ zero)
{
    __shared__ double p[MH_TPB];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * n_cols;
    double s = 0.0;
    for (uint32_t c = tid; c < n_cols; c += MH_TPB) {
        const uint32_t t = total[base + c];
        if (t == 0) {
            atomicOr(zero, 1u);
            continue;
        }
        const double j = (double)shared[base + c] / (double)t;
        s += 2.0 * j / (1.0 + j);
    }
    p[tid] = s;
    __syncthreads();
    for (uint32_t d = MH_TPB / 2; d > 0; d >>= 1) {
        if (tid < d) p[tid] += p[tid + d];
        __syncthreads();
    }
    if (tid == 0) rowsum[blockIdx.x] = p[0];
}

}  // namespace
}  // namespace sw

struct sw_minhash {
    int device = 0;
    uint64_t n = 0, s = 0, k = 0, n_hashes = 0, max_len = 0;
    uint32_t hash_bits = 64;
    std::vector<uint64_t> off_host;    // [n + 1]
    sw::DevArray<uint64_t> off;        // [n + 1]
    sw::DevArray<uint64_t> h64;        // hash_bits == 64
    sw::DevArray<uint32_t> h32;        // hash_bits == 32
    uint64_t counters[4] = {};         // assemblies finished by the general route, candidates kept, largest candidate count, capacity
    double ms[2] = {};                 // hash + pre-select pass, selection (with the general route and the compaction)
};

namespace sw {
namespace {

void run_hash(const HashArgs &g, hipStream_t stream)
{
    const uint32_t blocks = launch_blocks(MH_BLOCKS_ENV);
    switch (g.k / 16) {
    case 0: launch_tiles(k_mh_hash<0>, g, blocks, stream); break;
    case 1: launch_tiles(k_mh_hash<1>, g, blocks, stream); break;
    default: launch_tiles(k_mh_hash<2>, g, blocks, stream); break;
    }
}

uint64_t byte_mask(uint32_t n_bytes) { return n_bytes >= 8 ? ~0ull : (1ull << (8 * n_bytes)) - 1; }

void check_k_s(uint64_t k, uint64_t s, uint64_t seed)
{
    if (k < 1 || k > 32) raise(SW_ERR_VALUE, "minhash: k-mer length must lie in 1..32 (got %llu)", (unsigned long long)k);
    if (s < 1 || s > 0xFFFFFFFFull) raise(SW_ERR_VALUE, "minhash: sketch size must lie in 1..2^32-1 (got %llu)", (unsigned long long)s);
    if (seed > 0xFFFFFFFFull) raise(SW_ERR_VALUE, "minhash: the seed is a 32-bit value (got %llu)", (unsigned long long)seed);
}

void batch_minhash(const sw_batch &b, uint32_t k, uint64_t S, uint32_t seed, hipStream_t stream, sw_minhash &o)
{
    const HostBatch &h = b.host;
    const uint64_t n_asm = h.n_assemblies;
    const size_t R = h.rec_len.size();
    if (n_asm > MH_MAX_BLOCKS) raise(SW_ERR_VALUE, "minhash: %llu assemblies exceed one launch (%u)", (unsigned long long)n_asm, MH_MAX_BLOCKS);
    if (R && !b.d_packed.p) raise(SW_ERR_VALUE, "minhash: the batch holds no packed bases (it must be resident)");
    const bool bits32 = k <= 16;
    // ---- the valid runs of length >= k, once per call (kmer_walk.hpp) ----
    RunTiles RT;
    build_run_tiles(h, k, "minhash", RT);
    const std::vector<uint32_t> &asm_tile_off = RT.asm_tile_off;
    const uint64_t n_runs = RT.n_runs;
    auto n_valid = [&](uint64_t a) { return RT.asm_kmers[a + 1] - RT.asm_kmers[a]; };

    // ---- thresholds.  An assembly keeps the hashes at or below T_a = lambda / n_valid_a of the hash range, lambda = 2 S + 256
    // expected candidates (the multiple 2, the floor 256: small S stays far from falling short); a range holds `cap` of them.
    // None of the three changes a result; they were chosen without a measurement (NOTES.md, "MinHash sketches and pair counts on the device"). ----
    const double lambda = 2.0 * (double)S + 256.0;
    uint64_t cap = 256;
    while ((double)cap < lambda + 8.0 * std::sqrt(lambda)) cap <<= 1;
    const bool lds_route = cap <= MH_SEL_MAX && n_runs > 0;   // a larger S: every assembly by the general route
    cap = std::min<uint64_t>(cap, MH_SEL_MAX);
    cap = std::max<uint64_t>(std::min<uint64_t>(cap, env_u64(SW_TEST_GETENV("SEQWIN_AMD_MH_CAND_CAP"), cap)), 1);
    uint32_t P = 1;
    while (P < cap) P <<= 1;
    std::vector<uint64_t> thr(n_asm), ub_off(n_asm + 1, 0);
    std::vector<uint8_t> whole(n_asm);
    const double range = bits32 ? 4294967296.0 : 18446744073709551616.0;
    for (uint64_t a = 0; a < n_asm; ++a) {
        const double frac = n_valid(a) ? lambda / (double)n_valid(a) : 1.0;
        whole[a] = frac >= 1.0;
        thr[a] = whole[a] ? ~0ull : (uint64_t)(frac * range);
        ub_off[a + 1] = ub_off[a] + std::min<uint64_t>(S, n_valid(a));
    }

    Event e0, e1, e2;
    SW_HIP(hipEventRecord(e0, stream));
    DevRunTiles runs(RT, b.d_packed.p, stream);
    DevArray<uint64_t> d_thr(n_asm), d_ub(n_asm + 1), d_tmp(ub_off[n_asm]);
    DevArray<uint32_t> d_len(n_asm);
    DevArray<uint8_t> d_whole(n_asm), d_fall(n_asm);
    DevArray<unsigned long long> d_cnt(n_asm + 1);   // [n_asm]: the general route's counter
    auto up = [&](void *dst, const void *src, size_t bytes) {
        if (bytes) SW_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    };
    up(d_thr.p, thr.data(), n_asm * 8);
    up(d_ub.p, ub_off.data(), (n_asm + 1) * 8);
    up(d_whole.p, whole.data(), n_asm);
    SW_HIP(hipMemsetAsync(d_cnt.p, 0, (n_asm + 1) * 8, stream));
    if (n_asm) SW_HIP(hipMemsetAsync(d_len.p, 0, n_asm * 4, stream));
    const uint32_t tl = k & 15u;
    HashArgs g{};
    g.thr = d_thr.p;
    g.k = k;
    g.seed = seed;
    g.bits32 = bits32 ? 1 : 0;
    g.m1 = byte_mask(std::min<uint32_t>(tl, 8));
    g.m2 = byte_mask(tl > 8 ? tl - 8 : 0);

    std::vector<uint8_t> fall(n_asm, 1);
    std::vector<unsigned long long> cnt(n_asm, 0);
    if (lds_route && n_asm) {
        DevArray<uint64_t> d_cand(n_asm * cap);
        g.v = runs.view(0, (uint32_t)RT.tiles);
        g.cnt = d_cnt.p;
        g.cand = d_cand.p;
        g.cap = cap;
        g.single = 0;
        run_hash(g, stream);
        SW_HIP(hipEventRecord(e1, stream));
        const size_t lds = (size_t)P * 8;
        SW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mh_select), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_mh_select, dim3((unsigned)n_asm), dim3(MH_TPB), lds, stream, d_cand.p, d_cnt.p, cap, d_whole.p, S, d_ub.p, d_tmp.p,
                           d_len.p, d_fall.p);
        SW_HIP(hipGetLastError());
        SW_HIP(hipMemcpyAsync(fall.data(), d_fall.p, n_asm, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipMemcpyAsync(cnt.data(), d_cnt.p, n_asm * 8, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
    } else {
        SW_HIP(hipEventRecord(e1, stream));
    }
    // ---- the general route: every assembly that fell short, once ----
    uint64_t n_general = 0;
    for (uint64_t a = 0; a < n_asm; ++a) {
        if (!fall[a]) continue;
        const uint64_t nv = n_valid(a);
        if (nv == 0) continue;   // (no k-mer: an empty sketch, d_len[a] = 0)
        ++n_general;
        DevArray<uint64_t> keys(nv), alt(nv);
        DevArray<uint32_t> d_fail(1);
        SW_HIP(hipMemsetAsync(d_cnt.p + n_asm, 0, 8, stream));
        SW_HIP(hipMemsetAsync(d_fail.p, 0, 4, stream));
        g.v = runs.view(asm_tile_off[a], asm_tile_off[a + 1]);
        g.cnt = d_cnt.p + n_asm;
        g.cand = keys.p;
        g.cap = nv;
        g.single = 1;
        run_hash(g, stream);
        uint64_t *kp = keys.p, *ap = alt.p;
        sort_keys64(kp, ap, nv, 0, bits32 ? 32 : 64, stream, d_fail.p);
        uint32_t failed = 0;
        SW_HIP(hipMemcpyAsync(&failed, d_fail.p, 4, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
        check_sort_failed(failed);
        hipLaunchKernelGGL(k_mh_take, dim3(1), dim3(MH_TPB), 0, stream, kp, nv, S, d_tmp.p + ub_off[a], d_len.p + a);
        SW_HIP(hipGetLastError());
        SW_HIP(hipStreamSynchronize(stream));   // (keys / alt go back to the pool behind the kernel)
    }
    // ---- CSR ----
    std::vector<uint32_t> len(n_asm, 0);
    if (n_asm) SW_HIP(hipMemcpyAsync(len.data(), d_len.p, n_asm * 4, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    o.off_host.assign(n_asm + 1, 0);
    for (uint64_t a = 0; a < n_asm; ++a) {
        o.off_host[a + 1] = o.off_host[a] + len[a];
        o.max_len = std::max<uint64_t>(o.max_len, len[a]);
    }
    o.n = n_asm;
    o.n_hashes = o.off_host[n_asm];
    o.off.alloc(n_asm + 1);
    up(o.off.p, o.off_host.data(), (n_asm + 1) * 8);
    if (bits32) {
        o.h32.alloc(o.n_hashes);
        if (n_asm) hipLaunchKernelGGL(k_mh_compact<uint32_t>, dim3((unsigned)n_asm), dim3(MH_TPB), 0, stream, d_tmp.p, d_ub.p, o.off.p, o.h32.p);
    } else {
        o.h64.alloc(o.n_hashes);
        if (n_asm) hipLaunchKernelGGL(k_mh_compact<uint64_t>, dim3((unsigned)n_asm), dim3(MH_TPB), 0, stream, d_tmp.p, d_ub.p, o.off.p, o.h64.p);
    }
    SW_HIP(hipGetLastError());
    SW_HIP(hipEventRecord(e2, stream));
    SW_HIP(hipStreamSynchronize(stream));
    uint64_t kept = 0, largest = 0;
    for (uint64_t a = 0; a < n_asm; ++a) {
        kept += std::min<uint64_t>(cnt[a], cap);
        largest = std::max<uint64_t>(largest, cnt[a]);
    }
    const uint64_t cn[4] = {n_general, kept, largest, cap};
    memcpy(o.counters, cn, sizeof cn);
    float ms = 0;
    SW_HIP(hipEventElapsedTime(&ms, e0, e1));
    o.ms[0] = ms;
    SW_HIP(hipEventElapsedTime(&ms, e1, e2));
    o.ms[1] = ms;
}

void check_block(const sw_minhash *h, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1)
{
    if (!h) raise(SW_ERR_VALUE, "minhash: a NULL handle");
    if (r0 > r1 || r1 > h->n || c0 > c1 || c1 > h->n)
        raise(SW_ERR_VALUE, "minhash: rows [%llu, %llu) x columns [%llu, %llu) lie outside the %llu sketches", (unsigned long long)r0,
              (unsigned long long)r1, (unsigned long long)c0, (unsigned long long)c1, (unsigned long long)h->n);
}

// the counts of a block into device arrays of (r1 - r0) * (c1 - c0) entries
void device_counts(const sw_minhash &h, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *d_shared, uint32_t *d_total, hipStream_t stream)
{
    const uint64_t nr = r1 - r0, nc = c1 - c0;
    if (!nr || !nc) return;
    const uint32_t col_tiles = (uint32_t)((nc + MH_PAIR_COLS - 1) / MH_PAIR_COLS);
    const size_t esz = h.hash_bits == 32 ? 4 : 8, row_bytes = h.max_len * esz;
    const bool in_lds = row_bytes <= MH_PAIR_LDS_BYTES;
    const size_t lds = in_lds ? std::max<size_t>(row_bytes, 8) : 8;
    const uint64_t rows_per = std::max<uint64_t>(launch_blocks(MH_BLOCKS_ENV) / col_tiles, 1);   // (col_tiles < 2^26: below 2^32 threads either way)
    for (uint64_t ra = 0; ra < nr; ra += rows_per) {
        const uint64_t rn = std::min<uint64_t>(rows_per, nr - ra);
        const dim3 grid((unsigned)(rn * col_tiles)), block(MH_TPB);
        const uint32_t rr = (uint32_t)(r0 + ra);
        uint32_t *sh = d_shared + ra * nc, *to = d_total + ra * nc;
        if (h.hash_bits == 32) {
            if (in_lds)
                hipLaunchKernelGGL((k_mh_pairs<uint32_t, true>), grid, block, lds, stream, h.off.p, h.h32.p, rr, (uint32_t)c0, (uint32_t)nc, col_tiles, h.s, sh, to);
            else
                hipLaunchKernelGGL((k_mh_pairs<uint32_t, false>), grid, block, lds, stream, h.off.p, h.h32.p, rr, (uint32_t)c0, (uint32_t)nc, col_tiles, h.s, sh, to);
        } else {
            if (in_lds)
                hipLaunchKernelGGL((k_mh_pairs<uint64_t, true>), grid, block, lds, stream, h.off.p, h.h64.p, rr, (uint32_t)c0, (uint32_t)nc, col_tiles, h.s, sh, to);
            else
                hipLaunchKernelGGL((k_mh_pairs<uint64_t, false>), grid, block, lds, stream, h.off.p, h.h64.p, rr, (uint32_t)c0, (uint32_t)nc, col_tiles, h.s, sh, to);
        }
        SW_HIP(hipGetLastError());
    }
    SW_HIP(hipGetLastError());
}

}  // namespace
}  // namespace sw

using namespace sw;

extern "C" {

int sw_batch_minhash(const sw_batch *batch, uint64_t k, uint64_t s, uint64_t seed, void *stream, sw_minhash **out)
{
    return guarded([&] {
        check_k_s(k, s, seed);
        if (!batch || !out) raise(SW_ERR_VALUE, "minhash: a NULL handle");
        require_device(batch->device, "the batch");
        StreamScope scope((hipStream_t)stream);
        std::unique_ptr<sw_minhash> o(new sw_minhash);
        o->device = batch->device;
        o->k = k;
        o->s = s;
        o->hash_bits = k <= 16 ? 32 : 64;
        batch_minhash(*batch, (uint32_t)k, s, (uint32_t)seed, (hipStream_t)stream, *o);
        *out = o.release();
    });
}

int sw_minhash_from_sketches(const uint64_t *offsets, const uint64_t *hashes, uint64_t n, uint64_t s, uint64_t hash_bits, sw_minhash **out)
{
    return guarded([&] {
        if (!out || !offsets) raise(SW_ERR_VALUE, "minhash: a NULL array");
        if (hash_bits != 32 && hash_bits != 64) raise(SW_ERR_VALUE, "minhash: hash_bits must be 32 or 64 (got %llu)", (unsigned long long)hash_bits);
        check_k_s(1, s, 0);
        if (n >= 0xFFFFFFFFull) raise(SW_ERR_VALUE, "minhash: %llu sketches exceed 32-bit indices", (unsigned long long)n);
        if (offsets[0] != 0) raise(SW_ERR_VALUE, "minhash: offsets must start at 0");
        uint64_t max_len = 0;
        for (uint64_t a = 0; a < n; ++a) {
            if (offsets[a] > offsets[a + 1]) raise(SW_ERR_VALUE, "minhash: offsets must be non-decreasing (sketch %llu)", (unsigned long long)a);
            const uint64_t len = offsets[a + 1] - offsets[a];
            if (len > s) raise(SW_ERR_VALUE, "minhash: sketch %llu holds %llu values, more than s = %llu", (unsigned long long)a, (unsigned long long)len, (unsigned long long)s);
            max_len = std::max(max_len, len);
        }
        const uint64_t nh = offsets[n];
        if (nh && !hashes) raise(SW_ERR_VALUE, "minhash: a NULL array");
        for (uint64_t a = 0; a < n; ++a)
            for (uint64_t i = offsets[a]; i < offsets[a + 1]; ++i) {
                if (i > offsets[a] && !(hashes[i - 1] < hashes[i]))
                    raise(SW_ERR_VALUE, "minhash: sketch %llu is not strictly ascending", (unsigned long long)a);
                if (hash_bits == 32 && hashes[i] > 0xFFFFFFFFull)
                    raise(SW_ERR_VALUE, "minhash: sketch %llu holds a value above 2^32 - 1 in a 32-bit sketch", (unsigned long long)a);
            }
        std::unique_ptr<sw_minhash> o(new sw_minhash);
        SW_HIP(hipGetDevice(&o->device));
        o->n = n;
        o->s = s;
        o->hash_bits = (uint32_t)hash_bits;
        o->n_hashes = nh;
        o->max_len = max_len;
        o->off_host.assign(offsets, offsets + n + 1);
        o->off.alloc(n + 1);
        SW_HIP(hipMemcpy(o->off.p, offsets, (n + 1) * 8, hipMemcpyHostToDevice));
        if (hash_bits == 32) {
            std::vector<uint32_t> h32(hashes, hashes + nh);
            o->h32.alloc(nh);
            if (nh) SW_HIP(hipMemcpy(o->h32.p, h32.data(), nh * 4, hipMemcpyHostToDevice));
        } else {
            o->h64.alloc(nh);
            if (nh) SW_HIP(hipMemcpy(o->h64.p, hashes, nh * 8, hipMemcpyHostToDevice));
        }
        *out = o.release();
    });
}

int sw_minhash_sizes(const sw_minhash *h, uint64_t *n, uint64_t *n_hashes, uint64_t *s, uint64_t *hash_bits)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "minhash: a NULL handle");
        if (n) *n = h->n;
        if (n_hashes) *n_hashes = h->n_hashes;
        if (s) *s = h->s;
        if (hash_bits) *hash_bits = h->hash_bits;
    });
}

int sw_minhash_export(const sw_minhash *h, uint64_t *offsets, uint64_t *hashes)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "minhash: a NULL handle");
        if (offsets) memcpy(offsets, h->off_host.data(), (h->n + 1) * 8);
        if (!hashes || !h->n_hashes) return;
        require_device(h->device, "the sketches");
        if (h->hash_bits == 32) {
            std::vector<uint32_t> h32(h->n_hashes);
            SW_HIP(hipMemcpy(h32.data(), h->h32.p, h->n_hashes * 4, hipMemcpyDeviceToHost));
            for (uint64_t i = 0; i < h->n_hashes; ++i) hashes[i] = h32[i];
        } else {
            SW_HIP(hipMemcpy(hashes, h->h64.p, h->n_hashes * 8, hipMemcpyDeviceToHost));
        }
    });
}

int sw_minhash_counts(const sw_minhash *h, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *shared, uint32_t *total)
{
    return guarded([&] {
        check_block(h, r0, r1, c0, c1);
        const uint64_t np = (r1 - r0) * (c1 - c0);
        if (!np) return;
        if (!shared || !total) raise(SW_ERR_VALUE, "minhash: a NULL array");
        require_device(h->device, "the sketches");
        DevArray<uint32_t> d_sh(np), d_to(np);
        device_counts(*h, r0, r1, c0, c1, d_sh.p, d_to.p, 0);
        SW_HIP(hipMemcpy(shared, d_sh.p, np * 4, hipMemcpyDeviceToHost));
        SW_HIP(hipMemcpy(total, d_to.p, np * 4, hipMemcpyDeviceToHost));
    });
}

int sw_minhash_frac_rowsums(const sw_minhash *h, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, double *rowsums)
{
    return guarded([&] {
        check_block(h, r0, r1, c0, c1);
        const uint64_t nr = r1 - r0, nc = c1 - c0;
        if (!nr) return;
        if (!rowsums) raise(SW_ERR_VALUE, "minhash: a NULL array");
        if (nr > MH_MAX_BLOCKS) raise(SW_ERR_VALUE, "minhash: %llu rows exceed one launch (%u)", (unsigned long long)nr, MH_MAX_BLOCKS);
        if (!nc) {
            for (uint64_t r = 0; r < nr; ++r) rowsums[r] = 0.0;
            return;
        }
        require_device(h->device, "the sketches");
        DevArray<uint32_t> d_sh(nr * nc), d_to(nr * nc), d_zero(1);
        DevArray<double> d_sum(nr);
        SW_HIP(hipMemsetAsync(d_zero.p, 0, 4, 0));
        device_counts(*h, r0, r1, c0, c1, d_sh.p, d_to.p, 0);
        hipLaunchKernelGGL(k_mh_rowsum, dim3((unsigned)nr), dim3(MH_TPB), 0, 0, d_sh.p, d_to.p, (uint32_t)nc, d_sum.p, d_zero.p);
        SW_HIP(hipGetLastError());
        uint32_t zero = 0;
        SW_HIP(hipMemcpy(&zero, d_zero.p, 4, hipMemcpyDeviceToHost));
        if (zero) raise(SW_ERR_VALUE, "minhash: division by zero: a pair of two empty sketches (0 / 0) lies in the block");
        SW_HIP(hipMemcpy(rowsums, d_sum.p, nr * 8, hipMemcpyDeviceToHost));
    });
}

int sw_minhash_stats(const sw_minhash *h, uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (!h) raise(SW_ERR_VALUE, "minhash: a NULL handle");
        if (counters) memcpy(counters, h->counters, sizeof h->counters);
        if (ms) memcpy(ms, h->ms, sizeof h->ms);
    });
}

void sw_minhash_free(sw_minhash *h)
{
    delete h;
}

}  // extern "C"
