// kmer_walk.hpp -- every k-mer of a resident batch, once: the walk that k_mh_hash (minhash.hip), k_scr_probe (screen.hip) and
// k_hit_probe (hits.hip) share.  The valid runs of length >= k are cut into tiles of 1024 k-mers, ordered by assembly; a tile goes
// to a wave, a lane takes 16 consecutive k-mers of it, unpacks their 2-bit bases and rolls the forward and the reverse-complement
// word in registers.  Here: the host's run table and its device copy, the tile -> run search, the lane's roller, the wave's append
// to a cursor and the launch loop over a tile range.  What a kernel does with a k-mer stays in its file.  Device functions cannot
// be linked across translation units here, so the three files include this header.
#pragma once
#include "device.hpp"

namespace sw {
namespace {

constexpr uint32_t KW_TPB = 256, KW_WAVE = 64, KW_WPB = KW_TPB / KW_WAVE;
constexpr uint32_t KW_L = 16;                  // consecutive k-mers per lane
constexpr uint32_t KW_TILE = 1024;             // k-mers per wave: one tile lies inside one valid run
constexpr uint32_t KW_MAX_BLOCKS = MAX_LAUNCH_BLOCKS;
static_assert(KW_TILE == KW_WAVE * KW_L, "a tile is what the lanes of one wave take");

// ---- the valid runs of length >= k as tiles of KW_TILE k-mers, once per call (as get_plan takes its segments) ------------------------
struct RunTiles {
    std::vector<uint64_t> run_base;                 // batch-wide index of the run's first base
    std::vector<uint32_t> run_nk, run_asm, run_tile_off, run_rec, run_pos, asm_tile_off;   // run_rec / run_pos: the record and the run's place in it
    std::vector<uint64_t> asm_kmers;                // k-mers of the assemblies before a
    uint64_t tiles = 0, n_runs = 0;
};

// what: the caller's name in the two error messages
void build_run_tiles(const HostBatch &h, uint32_t k, const char *what, RunTiles &T)
{
    const uint64_t n_asm = h.n_assemblies;
    T.asm_tile_off.assign(n_asm + 1, 0);
    T.asm_kmers.assign(n_asm + 1, 0);
    uint64_t tiles = 0;
    for (uint64_t a = 0; a < n_asm; ++a) {
        T.asm_tile_off[a] = (uint32_t)tiles;
        T.asm_kmers[a + 1] = T.asm_kmers[a];
        for (uint32_t r = h.record_offsets[a]; r < h.record_offsets[a + 1]; ++r)
            for (uint32_t q = h.rec_run_off[r]; q < h.rec_run_off[r + 1]; ++q) {
                if (h.run_len[q] < k) continue;
                const uint32_t nk = h.run_len[q] - k + 1;
                T.run_base.push_back(h.rec_base[r] + h.run_pos[q]);
                T.run_nk.push_back(nk);
                T.run_asm.push_back((uint32_t)a);
                T.run_rec.push_back(r);
                T.run_pos.push_back(h.run_pos[q]);
                T.run_tile_off.push_back((uint32_t)tiles);
                tiles += ((uint64_t)nk + KW_TILE - 1) / KW_TILE;
                T.asm_kmers[a + 1] += nk;
                if (tiles >= 0xFFFFFFFFull) raise(SW_ERR_RUNTIME, "%s: the batch has more k-mers than one call takes (2^32 tiles of %u)", what, KW_TILE);
            }
    }
    T.asm_tile_off[n_asm] = (uint32_t)tiles;
    T.run_tile_off.push_back((uint32_t)tiles);
    T.tiles = tiles;
    T.n_runs = T.run_nk.size();
    if (T.n_runs >= 0xFFFFFFFFull) raise(SW_ERR_RUNTIME, "%s: %llu valid runs exceed 32-bit indices", what, (unsigned long long)T.n_runs);
}

// The run table as a kernel reads it, with the tiles of one launch
struct RunView {
    const uint32_t *packed;          // 16 bases per word, base i in bits [2 (i % 16), +2)
    const uint64_t *run_base;        // [n_runs] batch-wide index of the run's first base
    const uint32_t *run_nk;          // [n_runs] k-mers of the run (>= 1)
    const uint32_t *run_asm;         // [n_runs]
    const uint32_t *run_tile_off;    // [n_runs + 1] first tile of the run
    const uint32_t *run_rec, *run_pos;   // [n_runs] the run's record and its place in it (nullptr unless asked for)
    uint32_t n_runs;
    uint32_t tile_begin, tile_end;   // the tiles of this launch
};

// the device copies of a RunTiles, uploaded on `stream`; places: run_rec / run_pos too
struct DevRunTiles {
    DevArray<uint64_t> run_base;
    DevArray<uint32_t> run_nk, run_asm, run_tile_off, run_rec, run_pos;
    const uint32_t *packed;
    uint32_t n_runs;
    DevRunTiles(const RunTiles &T, const uint32_t *packed_bases, hipStream_t stream, bool places = false) : packed(packed_bases), n_runs((uint32_t)T.n_runs)
    {
        auto up = [&](auto &dst, const auto &src) {
            dst.alloc(src.size());
            if (src.size()) SW_HIP(hipMemcpyAsync(dst.p, src.data(), src.size() * sizeof(src[0]), hipMemcpyHostToDevice, stream));
        };
        up(run_base, T.run_base);
        up(run_nk, T.run_nk);
        up(run_asm, T.run_asm);
        up(run_tile_off, T.run_tile_off);
        if (places) {
            up(run_rec, T.run_rec);
            up(run_pos, T.run_pos);
        }
    }
    RunView view(uint32_t tile_begin = 0, uint32_t tile_end = 0) const
    {
        return RunView{packed, run_base.p, run_nk.p, run_asm.p, run_tile_off.p, run_rec.p, run_pos.p, n_runs, tile_begin, tile_end};
    }
};

// kern(g) over the tiles [g.v.tile_begin, g.v.tile_end) in launches of at most max_blocks workgroups (a launch holds fewer than 2^32
// threads, more wrap silently: the 15 000-genome set has 73 M tiles).  Returns the number of launches.
template <class Args> uint64_t launch_tiles(void (*kern)(Args), Args g, uint32_t max_blocks, hipStream_t stream)
{
    const uint64_t end = g.v.tile_end, step = (uint64_t)max_blocks * KW_WPB;
    uint64_t launches = 0;
    for (uint64_t t0 = g.v.tile_begin; t0 < end; t0 += step, ++launches) {
        g.v.tile_begin = (uint32_t)t0;
        g.v.tile_end = (uint32_t)std::min<uint64_t>(end, t0 + step);
        const uint64_t tiles = (uint64_t)g.v.tile_end - g.v.tile_begin;
        hipLaunchKernelGGL(kern, dim3((unsigned)((tiles + KW_WPB - 1) / KW_WPB)), dim3(KW_TPB), 0, stream, g);
        SW_HIP(hipGetLastError());
    }
    return launches;
}

// ---- device side ----------------------------------------------------------------------------------------------------------------
// Once per wave of a KW_TPB workgroup: its tile's run r, the lane's first k-mer in that run and how many of the KW_L from there on
// the run holds.  false: the wave has no tile in this launch (the whole wave).  lane = threadIdx.x % KW_WAVE, here and below: the
// caller's own value (k_scr_probe takes a VGPR more, and loses a wave per SIMD, if it is formed a second time in here)
__device__ __forceinline__ bool wave_tile(const RunView &v, uint32_t lane, uint32_t &r, uint64_t &first, uint32_t &n_mine)
{
    const uint32_t wave = threadIdx.x / KW_WAVE;
    const uint64_t tile64 = (uint64_t)v.tile_begin + (uint64_t)blockIdx.x * KW_WPB + wave;
    if (tile64 >= v.tile_end) return false;
    const uint32_t tile = (uint32_t)tile64;
    uint32_t lo = 0, hi = v.n_runs;     // the last run whose first tile is <= tile
    while (lo + 1 < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (v.run_tile_off[mid] <= tile) lo = mid; else hi = mid;
    }
    r = lo;
    const uint32_t nk = v.run_nk[r];
    first = (uint64_t)(tile - v.run_tile_off[r]) * KW_TILE + (uint64_t)lane * KW_L;
    n_mine = first < nk ? (uint32_t)(nk - first < KW_L ? nk - first : KW_L) : 0;
    return true;
}

// A lane's reader of consecutive bases: made for a k by every lane, started at a base by the lanes that have k-mers.  After k calls
// of roll(), fwd is the k-mer that ends at the last base read (first base most significant: integer order = byte-string order,
// A < C < G < T) and rev its reverse complement; the caller chooses between them.  A lane that takes n k-mers from pos0 on reads
// bases [pos0, pos0 + k - 1 + n), all inside its run.
struct KmerRoller {
    const uint32_t *packed;
    uint64_t pos = 0, fwd = 0, rev = 0, mask;
    uint32_t w = 0, left = 0, sh;
    __device__ __forceinline__ KmerRoller(const uint32_t *packed_bases, uint32_t k)
        : packed(packed_bases), mask(k >= 32 ? ~0ull : (1ull << (2 * k)) - 1), sh(2 * (k - 1))
    {
    }
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
        const uint64_t c = w & 3u;
        w >>= 2;
        --left;
        ++pos;
        fwd = ((fwd << 2) | c) & mask;
        rev = (rev >> 2) | ((3 - c) << sh);
    }
};

// The wave's lanes append `count` elements each behind *cursor: the counts scanned, the wave's range claimed by lane 0 with one
// atomic.  base: where the wave's range starts; total: its length (0: nothing was claimed, base means nothing); offset: the
// lane's place in it.  Whether base + total still fits is the caller's rule.  The whole wave calls it.
struct WaveRange {
    unsigned long long base;
    uint32_t total, offset;
};

__device__ __forceinline__ WaveRange wave_append(unsigned long long *cursor, uint32_t lane, uint32_t count)
{
    uint32_t incl = count;
    for (uint32_t d = 1; d < KW_WAVE; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, KW_WAVE);
        if (lane >= d) incl += o;
    }
    const uint32_t total = __shfl(incl, KW_WAVE - 1, KW_WAVE);
    if (!total) return WaveRange{0, 0, 0};   // (uniform)
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(cursor, (unsigned long long)total);
    base = __shfl(base, 0, KW_WAVE);
    return WaveRange{base, total, incl - count};
}

}  // namespace
}  // namespace sw
