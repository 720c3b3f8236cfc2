// subgraph.hip -- kmers._get_subgraphs (src/seqwin/kmers.py:176-312) on the device: greedy seed expansion of low-penalty
// subgraphs over a filtered index (sw_index_filter_graph), with the reference's result bit for bit.
//
// Two facts make the walk exact without a heap:
//   * the first rejection ends an expansion: nodes enter the frontier only when a node is accepted and the pops come in
//     non-decreasing (penalty, hash) order, so (sum + p) / (|sg| + 1) only grows from the first rejected pop on.  An expansion
//     is "take the least (penalty, hash) frontier node while the running average stays <= penalty_th and |sg| < max_nodes";
//   * random.shuffle depends on the length of the list only: the caller shuffles list(range(n)) and hands the permutation in.
//
// The walk is serial in the reference only through `used`.  Seed i's expansion reads `used` on T_i = {s} u N(sg_i), so it runs
// speculatively in rounds (see sw_index_subgraphs in include/seqwin_hip.h): a window of the next B unused seeds expands in
// parallel, one wave per seed, against `used` as it stood at the start of the round; every kept expansion claims its nodes with
// atomicMin(window position); seed i is valid iff no node of T_i carries a claim from a position < i; the longest valid prefix
// is committed, the first invalid seed opens the next round.  Window size 1 is the serial algorithm.
//
// Arithmetic: plain double + and / (the library builds with -ffp-contract=off), <= against the caller's threshold.
// (penalty, hash) orders as the 96-bit integer (penalty bits, rank): non-negative doubles order as their bit patterns and a
// node's rank in the hash-sorted filtered nodes orders as its hash (-0.0 is keyed as +0.0).
#include <cmath>
#include <cstring>  // rocprim's texture iterator needs ::memset declared first
#include <memory>

#include <rocprim/rocprim.hpp>

#include "device.hpp"

namespace sw {
namespace {

constexpr uint32_t SG_NONE = 0xFFFFFFFFu;        // no claim / no subgraph / a neighbour slot to skip (duplicate, self-loop)
constexpr int SG_WAVE = 64;
constexpr uint32_t SG_FCAP = 1024;               // frontier entries a wave keeps in LDS (12 B each)
constexpr uint32_t SG_SCAP = 128;                // subgraph nodes a wave keeps in LDS (>= max_nodes_cap = 100, config.py:148)
constexpr uint32_t SG_BMIN = 64, SG_BMAX = 4096, SG_B0 = 256;   // window sizes (adaptive, sw_index_subgraphs)
constexpr int SG_TPB = 256;
constexpr int SG_NCOUNTERS = 10;

inline unsigned sg_blocks(uint64_t n) { return (unsigned)((n + SG_TPB - 1) / SG_TPB); }

// Device-resident state of the walk: read back once per round (a few words), no per-seed host work.
struct SgState {
    unsigned long long cursor;         // next seed position (in the shuffled order)
    unsigned long long count;          // seeds in this round's window
    unsigned long long window_end;     // seed position after the window's last seed
    unsigned long long first_spill;    // least window position whose expansion left the LDS bounds (SG_NONE: none)
    unsigned long long first_invalid;  // least invalid window position (SG_NONE: none)
    unsigned long long n_sg, n_out;    // committed subgraphs, their nodes
    unsigned long long rounds, expansions, invalidated, skipped, kept, discarded, max_frontier, spilled;
    unsigned long long last_commit;    // committed prefix of the last round
};

struct Walk {
    const uint64_t *pbits;   // [n] penalty bit patterns (the f64 itself, as read by the reference)
    const uint64_t *off;     // [n + 1] CSR rows
    const uint32_t *nbr;     // [off[n]] neighbour ranks (SG_NONE: skip)
    const uint8_t *used;     // [n]
    double th;
    uint64_t max_nodes;      // UINT64_MAX: None
};

__device__ inline double as_f64(uint64_t b) { return __longlong_as_double((long long)b); }
__device__ inline uint64_t pkey(uint64_t b) { return b == 0x8000000000000000ull ? 0ull : b; }   // -0.0 orders as +0.0

__device__ inline uint32_t lower_bound_u64(const uint64_t *a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return (uint32_t)lo;
}

// ---- adjacency ------------------------------------------------------------------------------------------------------------
// Both directions of every edge as (src rank << 32 | dst rank); the endpoints' ranks by binary search in the sorted hashes.
__global__ void k_edge_keys(const sw_edge *edges, uint64_t m, const sw_node *nodes, uint64_t n, uint64_t *keys, uint32_t *era,
                            uint32_t *erb, unsigned int *err)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const uint64_t a = edges[e].first, b = edges[e].second;
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (nodes[mid].hash < a) lo = mid + 1; else hi = mid; }
    const uint64_t ra = lo;
    lo = 0; hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (nodes[mid].hash < b) lo = mid + 1; else hi = mid; }
    const uint64_t rb = lo;
    if (ra >= n || rb >= n || nodes[ra].hash != a || nodes[rb].hash != b) {
        atomicOr(err, 1u);
        keys[2 * e] = keys[2 * e + 1] = ~0ull;
        era[e] = erb[e] = SG_NONE;
        return;
    }
    keys[2 * e] = ra << 32 | rb;
    keys[2 * e + 1] = rb << 32 | ra;
    era[e] = (uint32_t)ra;
    erb[e] = (uint32_t)rb;
}

// off[r] = first key of source r (r in [0, n]); node penalties as bit patterns
__global__ void k_rows(const uint64_t *keys, uint64_t nk, const sw_node *nodes, uint64_t n, uint64_t *off, uint64_t *pbits)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    off[r] = lower_bound_u64(keys, nk, r << 32);
    if (r < n) {
        double p = nodes[r].penalty;
        uint64_t b;
        memcpy(&b, &p, 8);
        pbits[r] = b;
    }
}

// neighbour lists; a repeated (src, dst) and a self-loop become SG_NONE (the loop's node is in sg whenever it is looked at)
__global__ void k_nbrs(const uint64_t *keys, uint64_t nk, uint32_t *nbr)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nk) return;
    const uint64_t k = keys[j];
    const bool skip = (k >> 32) == (k & 0xFFFFFFFFull) || (j > 0 && keys[j - 1] == k);
    nbr[j] = skip ? SG_NONE : (uint32_t)k;
}

// seed flag: a node of the graph (an endpoint of an edge, self-loops included) with penalty <= th (kmers.py:243-245)
struct SeedFlag {
    const uint64_t *off;
    const uint64_t *pbits;
    double th;
    __host__ __device__ uint32_t operator()(uint64_t r) const
    {
#ifdef __HIP_DEVICE_COMPILE__
        return (off[r + 1] > off[r] && as_f64(pbits[r]) <= th) ? 1u : 0u;
#else
        return 0u;
#endif
    }
};

__global__ void k_seed_scatter(const uint64_t *off, const uint64_t *pbits, double th, uint64_t n, const uint32_t *cum, uint32_t *seeds)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    if (off[r + 1] > off[r] && as_f64(pbits[r]) <= th) seeds[cum[r] - 1] = (uint32_t)r;
}

// shuffled[i] = seeds[perm[i]] (what rng.shuffle does to the seed list, kmers.py:246); a bad permutation sets *err
__global__ void k_apply_perm(const uint32_t *seeds, const uint64_t *perm, uint64_t ns, uint32_t *seen, uint32_t *out, unsigned int *err)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const uint64_t p = perm[i];
    if (p >= ns || atomicExch(&seen[p], 1u) != 0u) {
        atomicOr(err, 2u);
        out[i] = seeds[0];
        return;
    }
    out[i] = seeds[p];
}

// ---- one expansion, one wave ---------------------------------------------------------------------------------------------
// fk / fr: frontier keys / ranks (cap entries), sg: the subgraph in acceptance order (scap entries).  SPILL: the arrays are the
// spill scratch in global memory (cap = scap = n: never full) and membership is a stamp per node; otherwise they are in LDS and
// membership is a scan of sg and the frontier.  Returns false if a bound was reached (the caller spills the expansion).
template <bool SPILL>
__device__ bool expand(const Walk &g, uint32_t s, uint64_t *fk, uint32_t *fr, uint32_t cap, uint32_t *sg, uint32_t scap,
                       uint32_t *stamp, uint32_t stamp_val, uint32_t *ns_out, uint32_t *nfmax_out)
{
    const int lane = threadIdx.x;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t ns = 1, nf = 0, nfmax = 0;
    double sum = as_f64(g.pbits[s]);
    if (lane == 0) {
        sg[0] = s;
        if (SPILL) stamp[s] = stamp_val;
    }
    __syncthreads();
    uint32_t u = s;
    for (;;) {
        if ((uint64_t)ns >= g.max_nodes) break;   // (the neighbours of the last node are read by the validation, not needed here)
        // bring in the neighbours of u that are in neither used, sg nor the frontier
        const uint64_t j1 = g.off[u + 1];
        for (uint64_t j0 = g.off[u]; j0 < j1; j0 += SG_WAVE) {
            const uint64_t j = j0 + lane;
            const uint32_t v = j < j1 ? g.nbr[j] : SG_NONE;
            bool add = v != SG_NONE && !g.used[v];
            if (add) {
                if (SPILL) {
                    add = stamp[v] != stamp_val;
                } else {
                    for (uint32_t i = 0; i < ns && add; ++i) add = sg[i] != v;
                    for (uint32_t i = 0; i < nf && add; ++i) add = fr[i] != v;
                }
            }
            const unsigned long long mask = __ballot(add);
            const uint32_t cnt = (uint32_t)__popcll(mask);
            if (nf + cnt > cap) return false;
            if (add) {
                const uint32_t at = nf + (uint32_t)__popcll(mask & lt);
                fk[at] = pkey(g.pbits[v]);
                fr[at] = v;
                if (SPILL) stamp[v] = stamp_val;
            }
            nf += cnt;
            __syncthreads();
        }
        nfmax = nf > nfmax ? nf : nfmax;
        if (nf == 0) break;
        // the least (penalty, hash) of the frontier
        uint64_t bk = ~0ull;
        uint32_t br = SG_NONE, bi = 0;
        for (uint32_t i = lane; i < nf; i += SG_WAVE) {
            const uint64_t k = fk[i];
            const uint32_t r = fr[i];
            if (k < bk || (k == bk && r < br)) { bk = k; br = r; bi = i; }
        }
        for (int d = SG_WAVE / 2; d; d >>= 1) {
            const uint64_t ok = __shfl_xor(bk, d, SG_WAVE);
            const uint32_t orr = __shfl_xor(br, d, SG_WAVE), oi = __shfl_xor(bi, d, SG_WAVE);
            if (ok < bk || (ok == bk && orr < br)) { bk = ok; br = orr; bi = oi; }
        }
        const double p = as_f64(g.pbits[br]);
        const double nsum = sum + p;
        if (!(nsum / (double)(ns + 1) <= g.th)) break;   // rejected: so is every later pop
        if (ns >= scap) return false;
        sum = nsum;
        __syncthreads();   // every lane has read the frontier before it changes
        if (lane == 0) {
            sg[ns] = br;
            fk[bi] = fk[nf - 1];
            fr[bi] = fr[nf - 1];
        }
        ++ns;
        --nf;
        __syncthreads();
        u = br;
    }
    *ns_out = ns;
    *nfmax_out = nfmax;
    return true;
}

struct Round {
    const uint32_t *seeds;   // [n_seeds] shuffled seed ranks
    uint64_t n_seeds;
    uint32_t *win_rank;      // [SG_BMAX]
    uint64_t *win_pos;       // [SG_BMAX]
    uint32_t *slots;         // [SG_BMAX * SG_SCAP] subgraphs of the window (LDS-sized expansions)
    uint32_t *len;           // [SG_BMAX]
    uint32_t *status;        // [SG_BMAX] 0: in slots, 1: over the LDS bounds, 2: in the spill scratch
    uint32_t *claim;         // [n]
    uint8_t *used;           // [n]
    uint64_t *sfk;           // spill scratch [n]
    uint32_t *sfr, *ssg, *stamp;   // [n]
    uint64_t *out_keys;      // [n] (subgraph << 32 | rank), commit order
    uint64_t *out_off;       // [n + 1]
    uint64_t min_nodes;
    uint32_t fcap;           // LDS frontier bound (SEQWIN_AMD_SG_LDS_CAP lowers it)
    SgState *st;
    uint64_t n;              // nodes (bound of out_keys / out_off: committed subgraphs are disjoint)
};

__device__ inline const uint32_t *sg_of(const Round &R, uint32_t j)
{
    return R.status[j] == 2 ? R.ssg : R.slots + (uint64_t)j * SG_SCAP;
}
__device__ inline uint32_t effective(const SgState *st)
{
    const uint64_t cnt = st->count, fs = st->first_spill;
    return (uint32_t)(fs < cnt ? fs + 1 : cnt);
}

// (a) the next B seeds not in used, in order (one wave)
__global__ void __launch_bounds__(SG_WAVE) k_window(Round R, uint32_t B)
{
    const int lane = threadIdx.x;
    const unsigned long long lt = (1ull << lane) - 1ull;
    SgState *st = R.st;
    const uint64_t cursor = st->cursor;
    uint32_t cnt = 0;
    uint64_t end = cursor;
    for (uint64_t base = cursor; base < R.n_seeds; base += SG_WAVE) {
        const uint64_t i = base + lane;
        const bool ok = i < R.n_seeds && !R.used[R.seeds[i]];
        const unsigned long long mask = __ballot(ok);
        const uint32_t pre = (uint32_t)__popcll(mask & lt), tot = (uint32_t)__popcll(mask);
        if (ok && cnt + pre < B) {
            R.win_rank[cnt + pre] = R.seeds[i];
            R.win_pos[cnt + pre] = i;
        }
        if (cnt + tot >= B) {
            const unsigned long long last = __ballot(ok && cnt + pre == B - 1);
            end = base + (uint64_t)(__ffsll((long long)last) - 1) + 1;
            cnt = B;
            break;
        }
        cnt += tot;
        end = base + SG_WAVE < R.n_seeds ? base + SG_WAVE : R.n_seeds;
    }
    if (lane == 0) {
        st->count = cnt;
        st->window_end = end;
        st->first_spill = SG_NONE;
        st->first_invalid = SG_NONE;
    }
}

// (b) expand every seed of the window against `used` as it stood at the start of the round (one wave per seed, LDS)
__global__ void __launch_bounds__(SG_WAVE) k_expand(Walk g, Round R)
{
    __shared__ uint64_t fk[SG_FCAP];
    __shared__ uint32_t fr[SG_FCAP];
    __shared__ uint32_t sg[SG_SCAP];
    const uint32_t j = blockIdx.x;
    if (j >= R.st->count) return;
    uint32_t ns = 0, nfmax = 0;
    const bool ok = expand<false>(g, R.win_rank[j], fk, fr, R.fcap, sg, SG_SCAP, nullptr, 0, &ns, &nfmax);
    if (!ok) {
        if (threadIdx.x == 0) {
            R.status[j] = 1;
            atomicMin(&R.st->first_spill, (unsigned long long)j);
        }
        return;
    }
    uint32_t *dst = R.slots + (uint64_t)j * SG_SCAP;
    for (uint32_t i = threadIdx.x; i < ns; i += SG_WAVE) dst[i] = sg[i];
    if (threadIdx.x == 0) {
        R.len[j] = ns;
        R.status[j] = 0;
        atomicMax(&R.st->max_frontier, (unsigned long long)nfmax);
    }
}

// the first expansion that left the LDS bounds, again with the spill scratch (the window ends at it this round)
__global__ void __launch_bounds__(SG_WAVE) k_spill(Walk g, Round R, uint32_t n)
{
    SgState *st = R.st;
    const uint64_t fs = st->first_spill;
    if (fs >= st->count) return;
    const uint32_t j = (uint32_t)fs;
    const uint32_t stamp_val = (uint32_t)st->spilled + 1u;
    __syncthreads();
    uint32_t ns = 0, nfmax = 0;
    expand<true>(g, R.win_rank[j], R.sfk, R.sfr, n, R.ssg, n, R.stamp, stamp_val, &ns, &nfmax);
    if (threadIdx.x == 0) {
        R.len[j] = ns;
        R.status[j] = 2;
        st->spilled = stamp_val;
        atomicMax(&st->max_frontier, (unsigned long long)nfmax);
    }
}

// (c) kept expansions claim their nodes
__global__ void __launch_bounds__(SG_WAVE) k_claim(Round R)
{
    const uint32_t j = blockIdx.x;
    if (j >= effective(R.st)) return;
    const uint32_t L = R.len[j];
    if ((uint64_t)L < R.min_nodes) return;
    const uint32_t *sg = sg_of(R, j);
    for (uint32_t i = threadIdx.x; i < L; i += SG_WAVE) atomicMin(&R.claim[sg[i]], j);
}

// (d) seed j is valid iff no node of {s} u N(sg_j) carries a claim from a position < j
__global__ void __launch_bounds__(SG_WAVE) k_validate(Walk g, Round R)
{
    const uint32_t j = blockIdx.x;
    if (j == 0 || j >= effective(R.st)) return;
    const uint32_t *sg = sg_of(R, j);
    const uint32_t L = R.len[j];
    bool bad = R.claim[R.win_rank[j]] < j;
    for (uint32_t i = 0; i < L && !bad; ++i) {
        const uint32_t u = sg[i];
        const uint64_t j1 = g.off[u + 1];
        for (uint64_t k0 = g.off[u]; k0 < j1; k0 += SG_WAVE) {
            const uint64_t k = k0 + threadIdx.x;
            const uint32_t v = k < j1 ? g.nbr[k] : SG_NONE;
            const bool b = v != SG_NONE && R.claim[v] < j;
            if (__ballot(b)) { bad = true; break; }
        }
        if ((i & 15) == 15 && R.st->first_invalid < j) break;   // an earlier position is invalid already: j is not committed
    }
    if (bad && threadIdx.x == 0) atomicMin(&R.st->first_invalid, (unsigned long long)j);
}

// (e) commit the longest valid prefix in window order, reset the claims, advance the cursor (one workgroup)
__global__ void __launch_bounds__(SG_TPB) k_commit(Round R)
{
    __shared__ uint32_t node_off[SG_BMAX], sg_off[SG_BMAX];
    __shared__ uint32_t part_n[SG_TPB], part_s[SG_TPB];
    SgState *st = R.st;
    const uint32_t t = threadIdx.x;
    const uint32_t cnt = (uint32_t)st->count, eff = effective(st);
    const uint64_t fi = st->first_invalid;
    const uint32_t P = fi < eff ? (uint32_t)fi : eff;
    const uint64_t n_sg0 = st->n_sg, n_out0 = st->n_out;
    // exclusive offsets (nodes, subgraphs) of the kept expansions of the prefix
    const uint32_t C = (P + SG_TPB - 1) / SG_TPB;
    uint32_t an = 0, as = 0;
    for (uint32_t j = t * C; j < (t + 1) * C && j < P; ++j)
        if ((uint64_t)R.len[j] >= R.min_nodes) { an += R.len[j]; ++as; }
    part_n[t] = an;
    part_s[t] = as;
    __syncthreads();
    for (uint32_t d = 1; d < SG_TPB; d <<= 1) {
        const uint32_t xn = t >= d ? part_n[t - d] : 0, xs = t >= d ? part_s[t - d] : 0;
        __syncthreads();
        part_n[t] += xn;
        part_s[t] += xs;
        __syncthreads();
    }
    an = part_n[t] - an;
    as = part_s[t] - as;
    for (uint32_t j = t * C; j < (t + 1) * C && j < P; ++j) {
        node_off[j] = an;
        sg_off[j] = as;
        if ((uint64_t)R.len[j] >= R.min_nodes) { an += R.len[j]; ++as; }
    }
    __syncthreads();
    const uint32_t tot_n = part_n[SG_TPB - 1], tot_s = part_s[SG_TPB - 1];
    const uint32_t wave = t / SG_WAVE, lane = t % SG_WAVE;
    for (uint32_t j = wave; j < eff; j += SG_TPB / SG_WAVE) {
        const uint32_t L = R.len[j];
        if ((uint64_t)L < R.min_nodes) continue;
        const uint32_t *sg = sg_of(R, j);
        const bool commit = j < P;
        const uint64_t s_id = n_sg0 + (commit ? sg_off[j] : 0), base = n_out0 + (commit ? node_off[j] : 0);
        for (uint32_t i = lane; i < L; i += SG_WAVE) {
            const uint32_t v = sg[i];
            if (commit && base + i < R.n) {
                R.used[v] = 1;
                R.out_keys[base + i] = s_id << 32 | v;
            }
            R.claim[v] = SG_NONE;
        }
        if (commit && lane == 0 && s_id < R.n) R.out_off[s_id + 1] = base + L;
    }
    if (t == 0) {
        const uint64_t cur0 = st->cursor, cur = P < cnt ? R.win_pos[P] : st->window_end;
        st->n_sg = n_sg0 + tot_s;
        st->n_out = n_out0 + tot_n;
        st->rounds += 1;
        st->expansions += eff;
        st->invalidated += eff - P;
        st->kept += tot_s;
        st->discarded += P - tot_s;
        st->skipped += (cur - cur0) - P;
        st->cursor = cur;
        st->last_commit = P;
    }
}

// ---- after the walk ------------------------------------------------------------------------------------------------------
__global__ void k_sg_nodes(const uint64_t *keys, uint64_t n_out, const sw_node *nodes, uint64_t *hashes, uint32_t *sg_id)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const uint64_t k = keys[i];
    const uint32_t v = (uint32_t)k;
    hashes[i] = nodes[v].hash;
    sg_id[v] = (uint32_t)(k >> 32);
}

struct UsedFlag {
    const uint8_t *used;
    __host__ __device__ uint32_t operator()(uint64_t r) const { return used[r] ? 1u : 0u; }
};

__global__ void k_used_hashes(const uint8_t *used, const uint32_t *cum, const sw_node *nodes, uint64_t n, uint64_t *out, uint64_t n_out)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n && used[r] && cum[r] - 1 < n_out) out[cum[r] - 1] = nodes[r].hash;
}

// edges with both endpoints in the same subgraph (nx_graph.subgraph(sg), markers.py:418): (subgraph << 32 | edge), any order
__global__ void k_induced(const uint32_t *era, const uint32_t *erb, uint64_t m, const uint32_t *sg_id, uint64_t *keys,
                          unsigned long long *n_ie)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const uint32_t a = sg_id[era[e]], b = sg_id[erb[e]];
    if (a == SG_NONE || a != b) return;
    const unsigned long long at = atomicAdd(n_ie, 1ull);
    keys[at] = (uint64_t)a << 32 | e;
}

__global__ void k_induced_rows(const uint64_t *keys, uint64_t n_ie, const sw_edge *edges, sw_edge *out, uint64_t *ie_off, uint64_t n_sg)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_ie) out[i] = edges[(uint32_t)keys[i]];
    if (i <= n_sg) ie_off[i] = lower_bound_u64(keys, n_ie, i << 32);
}

template <class InIt, class T>
void scan_inclusive(InIt in, T *out, size_t n, hipStream_t stream)
{
    size_t tmp_bytes = 0;
    SW_HIP(rocprim::inclusive_scan(nullptr, tmp_bytes, in, out, n, rocprim::plus<T>(), stream));
    DevArray<unsigned char> tmp(tmp_bytes);
    SW_HIP(rocprim::inclusive_scan(tmp.p, tmp_bytes, in, out, n, rocprim::plus<T>(), stream));
}

void sort_u64(DevArray<uint64_t> &keys, uint64_t n, unsigned end_bit, hipStream_t stream)
{
    if (n < 2) return;
    DevArray<uint64_t> alt(n);
    DevArray<uint32_t> fail(1);
    SW_HIP(hipMemsetAsync(fail.p, 0, 4, stream));
    uint64_t *k = keys.p, *a = alt.p;
    sort_keys64(k, a, n, 0, end_bit, stream, fail.p);
    uint32_t f = 0;
    SW_HIP(hipMemcpyAsync(&f, fail.p, 4, hipMemcpyDeviceToHost, stream));
    if (k != keys.p) SW_HIP(hipMemcpyAsync(keys.p, k, n * 8, hipMemcpyDeviceToDevice, stream));
    SW_HIP(hipStreamSynchronize(stream));
    check_sort_failed(f);
}

unsigned bit_width(uint64_t x)
{
    unsigned b = 0;
    while (x) { ++b; x >>= 1; }
    return b;
}

// Symmetric CSR of a filtered index, and its seeds in rank order.
struct Csr {
    uint64_t n = 0, m = 0;
    DevArray<uint64_t> off, pbits;
    DevArray<uint32_t> nbr, era, erb;
    void build(const sw_index &f, hipStream_t stream)
    {
        if (f.edges_hold_ranks) raise(SW_ERR_VALUE, "the index's edges hold ranks, not hashes (a slice before sw_index_edge_hash_attach)");
        n = f.n_nodes;
        m = f.n_edges;
        if (n >= SG_NONE || m >= (1ull << 31)) raise(SW_ERR_VALUE, "subgraphs: %llu nodes / %llu edges exceed the 32-bit ranks of the walk",
                                                     (unsigned long long)n, (unsigned long long)m);
        off.alloc(n + 1);
        pbits.alloc(n);
        era.alloc(m);
        erb.alloc(m);
        const uint64_t nk = 2 * m;
        nbr.alloc(nk);
        DevArray<uint64_t> keys(nk);
        DevArray<unsigned int> err(1);
        SW_HIP(hipMemsetAsync(err.p, 0, 4, stream));
        if (m) hipLaunchKernelGGL(k_edge_keys, dim3(sg_blocks(m)), dim3(SG_TPB), 0, stream, f.edges.p, m, f.nodes.p, n, keys.p, era.p, erb.p, err.p);
        SW_HIP(hipGetLastError());
        unsigned int e = 0;
        SW_HIP(hipMemcpyAsync(&e, err.p, 4, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
        if (e) raise(SW_ERR_VALUE, "subgraphs: an edge endpoint is not among the nodes");
        sort_u64(keys, nk, std::min(64u, 32 + std::max(1u, bit_width(n))), stream);
        hipLaunchKernelGGL(k_rows, dim3(sg_blocks(n + 1)), dim3(SG_TPB), 0, stream, keys.p, nk, f.nodes.p, n, off.p, pbits.p);
        if (nk) hipLaunchKernelGGL(k_nbrs, dim3(sg_blocks(nk)), dim3(SG_TPB), 0, stream, keys.p, nk, nbr.p);
        SW_HIP(hipGetLastError());
        SW_HIP(hipStreamSynchronize(stream));   // (keys is released under the null stream: ordered anyway)
    }
    // seeds in rank order; returns their number
    uint64_t seeds(double th, DevArray<uint32_t> &out, hipStream_t stream)
    {
        if (n == 0) { out.alloc(0); return 0; }
        DevArray<uint32_t> cum(n);
        scan_inclusive(rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), SeedFlag{off.p, pbits.p, th}), cum.p, n,
                       stream);
        uint32_t ns = 0;
        SW_HIP(hipMemcpyAsync(&ns, cum.p + (n - 1), 4, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
        out.alloc(ns);
        if (ns) hipLaunchKernelGGL(k_seed_scatter, dim3(sg_blocks(n)), dim3(SG_TPB), 0, stream, off.p, pbits.p, th, n, cum.p, out.p);
        SW_HIP(hipGetLastError());
        SW_HIP(hipStreamSynchronize(stream));
        return ns;
    }
};

}  // namespace
}  // namespace sw

struct sw_subgraphs {
    int device = 0;
    uint64_t n_nodes = 0, n_sg = 0, n_out = 0, n_ie = 0;
    sw::DevArray<uint64_t> offsets, hashes, ie_offsets, used_hashes;
    sw::DevArray<sw_edge> ie_edges;
    sw::DevArray<uint8_t> used;
    uint64_t counters[sw::SG_NCOUNTERS] = {};
    double ms[3] = {};
};

namespace sw {
namespace {

void run_subgraphs(const sw_index &f, double th, uint64_t min_nodes, uint64_t max_nodes, const uint64_t *perm_host, uint64_t n_seeds_in,
                   sw_subgraphs &o)
{
    hipStream_t stream = 0;
    Event e0, e1, e2, e3;
    SW_HIP(hipEventRecord(e0, stream));
    Csr g;
    g.build(f, stream);
    DevArray<uint32_t> seeds_sorted;
    const uint64_t ns = g.seeds(th, seeds_sorted, stream);
    if (ns != n_seeds_in)
        raise(SW_ERR_VALUE, "subgraphs: the permutation has %llu entries, the graph has %llu seeds at penalty_th = %.17g",
              (unsigned long long)n_seeds_in, (unsigned long long)ns, th);
    const uint64_t n = g.n;
    o.device = f.device;
    o.n_nodes = n;
    o.used.alloc(n);
    if (n) SW_HIP(hipMemsetAsync(o.used.p, 0, n, stream));
    DevArray<uint32_t> seeds(ns);
    if (ns) {
        DevArray<uint64_t> d_perm(ns);
        DevArray<uint32_t> seen(ns);
        DevArray<unsigned int> err(1);
        SW_HIP(hipMemcpyAsync(d_perm.p, perm_host, ns * 8, hipMemcpyHostToDevice, stream));
        SW_HIP(hipMemsetAsync(seen.p, 0, ns * 4, stream));
        SW_HIP(hipMemsetAsync(err.p, 0, 4, stream));
        hipLaunchKernelGGL(k_apply_perm, dim3(sg_blocks(ns)), dim3(SG_TPB), 0, stream, seeds_sorted.p, d_perm.p, ns, seen.p, seeds.p, err.p);
        SW_HIP(hipGetLastError());
        unsigned int e = 0;
        SW_HIP(hipMemcpyAsync(&e, err.p, 4, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
        if (e) raise(SW_ERR_VALUE, "subgraphs: seed_perm is not a permutation of 0 .. %llu", (unsigned long long)(ns - 1));
    }
    SW_HIP(hipEventRecord(e1, stream));

    // ---- the walk, in rounds ----
    const uint64_t fixed_b = env_u64(SW_TEST_GETENV("SEQWIN_AMD_SG_WINDOW"), 0);
    const uint64_t fcap_env = env_u64(SW_TEST_GETENV("SEQWIN_AMD_SG_LDS_CAP"), SG_FCAP);
    DevArray<uint32_t> win_rank(SG_BMAX), len(SG_BMAX), status(SG_BMAX), slots((uint64_t)SG_BMAX * SG_SCAP), claim(n), sfr(n), ssg(n), stamp(n);
    DevArray<uint64_t> win_pos(SG_BMAX), sfk(n), out_keys(n), out_off(n + 1);
    DevArray<SgState> st(1);
    SgState h{};
    h.first_spill = h.first_invalid = SG_NONE;
    SW_HIP(hipMemcpyAsync(st.p, &h, sizeof h, hipMemcpyHostToDevice, stream));
    if (n) {
        SW_HIP(hipMemsetAsync(claim.p, 0xFF, n * 4, stream));
        SW_HIP(hipMemsetAsync(stamp.p, 0, n * 4, stream));
    }
    SW_HIP(hipMemsetAsync(out_off.p, 0, 8, stream));
    Round R{seeds.p, ns, win_rank.p, win_pos.p, slots.p, len.p, status.p, claim.p, o.used.p, sfk.p, sfr.p, ssg.p, stamp.p,
            out_keys.p, out_off.p, min_nodes, (uint32_t)std::min<uint64_t>(std::max<uint64_t>(fcap_env, 1), SG_FCAP), st.p, n};
    Walk w{g.pbits.p, g.off.p, g.nbr.p, o.used.p, th, max_nodes};
    // Window size: fixed by SEQWIN_AMD_SG_WINDOW (tests), else adaptive -- start at 256; a round that commits its whole window
    // doubles it, a round cut short at prefix P takes 2 P (the conflict distance just seen, with room to grow); kept in
    // [64, 4096]: below 64 waves a round costs its launches whatever it holds, 4096 waves fill the device several times over.
    uint64_t B = fixed_b ? std::min<uint64_t>(fixed_b, SG_BMAX) : SG_B0;
    while (h.cursor < ns) {
        hipLaunchKernelGGL(k_window, dim3(1), dim3(SG_WAVE), 0, stream, R, (uint32_t)B);
        hipLaunchKernelGGL(k_expand, dim3((unsigned)B), dim3(SG_WAVE), 0, stream, w, R);
        hipLaunchKernelGGL(k_spill, dim3(1), dim3(SG_WAVE), 0, stream, w, R, (uint32_t)n);
        hipLaunchKernelGGL(k_claim, dim3((unsigned)B), dim3(SG_WAVE), 0, stream, R);
        hipLaunchKernelGGL(k_validate, dim3((unsigned)B), dim3(SG_WAVE), 0, stream, w, R);
        hipLaunchKernelGGL(k_commit, dim3(1), dim3(SG_TPB), 0, stream, R);
        SW_HIP(hipGetLastError());
        SW_HIP(hipMemcpyAsync(&h, st.p, sizeof h, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
        if (!fixed_b) {
            if (h.last_commit >= h.count) B = std::min<uint64_t>(2 * B, SG_BMAX);
            else B = std::min<uint64_t>(std::max<uint64_t>(2 * h.last_commit, SG_BMIN), SG_BMAX);
        }
    }
    SW_HIP(hipEventRecord(e2, stream));

    // ---- results: subgraph CSR (hashes ascending inside each), used mask and hashes, induced edges ----
    if (h.n_out > n || h.n_sg > n) raise(SW_ERR_RUNTIME, "subgraphs: %llu committed nodes in %llu subgraphs over %llu nodes (overlap)",
                                        h.n_out, h.n_sg, (unsigned long long)n);
    o.n_sg = h.n_sg;
    o.n_out = h.n_out;
    const unsigned kb = 32 + std::max(1u, bit_width(o.n_sg));
    sort_u64(out_keys, o.n_out, std::min(kb, 64u), stream);
    o.offsets.alloc(o.n_sg + 1);
    SW_HIP(hipMemcpyAsync(o.offsets.p, out_off.p, (o.n_sg + 1) * 8, hipMemcpyDeviceToDevice, stream));
    o.hashes.alloc(o.n_out);
    DevArray<uint32_t> sg_id(n);
    if (n) SW_HIP(hipMemsetAsync(sg_id.p, 0xFF, n * 4, stream));
    if (o.n_out)
        hipLaunchKernelGGL(k_sg_nodes, dim3(sg_blocks(o.n_out)), dim3(SG_TPB), 0, stream, out_keys.p, o.n_out, f.nodes.p, o.hashes.p, sg_id.p);
    o.used_hashes.alloc(o.n_out);
    if (o.n_out) {
        DevArray<uint32_t> cum(n);
        scan_inclusive(rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), UsedFlag{o.used.p}), cum.p, n, stream);
        hipLaunchKernelGGL(k_used_hashes, dim3(sg_blocks(n)), dim3(SG_TPB), 0, stream, o.used.p, cum.p, f.nodes.p, n, o.used_hashes.p, o.n_out);
        SW_HIP(hipStreamSynchronize(stream));
    }
    DevArray<uint64_t> ie_keys(g.m);
    DevArray<unsigned long long> n_ie(1);
    SW_HIP(hipMemsetAsync(n_ie.p, 0, 8, stream));
    if (g.m && o.n_out)
        hipLaunchKernelGGL(k_induced, dim3(sg_blocks(g.m)), dim3(SG_TPB), 0, stream, g.era.p, g.erb.p, g.m, sg_id.p, ie_keys.p, n_ie.p);
    SW_HIP(hipGetLastError());
    unsigned long long nie = 0;
    SW_HIP(hipMemcpyAsync(&nie, n_ie.p, 8, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    o.n_ie = nie;
    sort_u64(ie_keys, o.n_ie, std::min(kb, 64u), stream);
    o.ie_edges.alloc(o.n_ie);
    o.ie_offsets.alloc(o.n_sg + 1);
    hipLaunchKernelGGL(k_induced_rows, dim3(sg_blocks(std::max(o.n_ie, o.n_sg + 1))), dim3(SG_TPB), 0, stream, ie_keys.p, o.n_ie, f.edges.p,
                       o.ie_edges.p, o.ie_offsets.p, o.n_sg);
    SW_HIP(hipGetLastError());
    SW_HIP(hipEventRecord(e3, stream));
    SW_HIP(hipStreamSynchronize(stream));
    float a = 0, b = 0, c = 0;
    SW_HIP(hipEventElapsedTime(&a, e0, e1));
    SW_HIP(hipEventElapsedTime(&b, e1, e2));
    SW_HIP(hipEventElapsedTime(&c, e2, e3));
    o.ms[0] = a;
    o.ms[1] = b;
    o.ms[2] = c;
    const uint64_t cn[SG_NCOUNTERS] = {ns, h.rounds, h.expansions, h.invalidated, h.skipped, h.kept, h.discarded, h.max_frontier, h.spilled, B};
    memcpy(o.counters, cn, sizeof cn);
}

}  // namespace

void subgraphs_csr(const sw_subgraphs *sg, int *device, uint64_t *n_sg, uint64_t *n_out, const uint64_t **offsets, const uint64_t **hashes)
{
    *device = sg->device;
    *n_sg = sg->n_sg;
    *n_out = sg->n_out;
    *offsets = sg->offsets.p;
    *hashes = sg->hashes.p;
}

}  // namespace sw

using namespace sw;

extern "C" {

int sw_index_from_arrays(const sw_node *nodes, uint64_t n_nodes, const sw_edge *edges, uint64_t n_edges, sw_index **out)
{
    return guarded([&] {
        for (uint64_t i = 0; i < n_nodes; ++i) {
            if (i && !(nodes[i - 1].hash < nodes[i].hash)) raise(SW_ERR_VALUE, "nodes must be strictly ascending by hash (node %llu)", (unsigned long long)i);
            const double p = nodes[i].penalty;
            if (!(p >= 0.0) || std::isinf(p)) raise(SW_ERR_VALUE, "node %llu: penalty %g is not a finite non-negative number", (unsigned long long)i, p);
        }
        std::unique_ptr<sw_index> o(new sw_index);
        SW_HIP(hipGetDevice(&o->device));
        o->n_nodes = n_nodes;
        o->n_edges = n_edges;
        o->kmers.alloc(0);
        o->nodes.alloc(n_nodes);
        o->edges.alloc(n_edges);
        if (n_nodes) SW_HIP(hipMemcpy(o->nodes.p, nodes, n_nodes * sizeof(sw_node), hipMemcpyHostToDevice));
        if (n_edges) SW_HIP(hipMemcpy(o->edges.p, edges, n_edges * sizeof(sw_edge), hipMemcpyHostToDevice));
        *out = o.release();
    });
}

int sw_index_subgraph_seeds(const sw_index *f, double penalty_th, uint64_t *n_seeds)
{
    return guarded([&] {
        require_device(f->device, "the index");
        Csr g;
        g.build(*f, 0);
        DevArray<uint32_t> s;
        *n_seeds = g.seeds(penalty_th, s, 0);
    });
}

int sw_index_subgraphs(const sw_index *f, double penalty_th, uint64_t min_nodes, uint64_t max_nodes, const uint64_t *seed_perm,
                       uint64_t n_seeds, sw_subgraphs **out)
{
    return guarded([&] {
        require_device(f->device, "the index");
        if (n_seeds && !seed_perm) raise(SW_ERR_VALUE, "seed_perm is NULL");
        std::unique_ptr<sw_subgraphs> o(new sw_subgraphs);
        run_subgraphs(*f, penalty_th, min_nodes, max_nodes, seed_perm, n_seeds, *o);
        *out = o.release();
    });
}

int sw_subgraphs_sizes(const sw_subgraphs *sg, uint64_t *n_subgraphs, uint64_t *n_sg_nodes, uint64_t *n_induced_edges, uint64_t *n_nodes)
{
    return guarded([&] {
        if (n_subgraphs) *n_subgraphs = sg->n_sg;
        if (n_sg_nodes) *n_sg_nodes = sg->n_out;
        if (n_induced_edges) *n_induced_edges = sg->n_ie;
        if (n_nodes) *n_nodes = sg->n_nodes;
    });
}

int sw_subgraphs_export(const sw_subgraphs *sg, uint64_t *offsets, uint64_t *hashes, uint64_t *edge_offsets, sw_edge *edges,
                        uint8_t *used_mask, uint64_t *used_hashes)
{
    return guarded([&] {
        require_device(sg->device, "the subgraphs");
        struct { void *dst; const void *src; uint64_t bytes; } c[6] = {
            {offsets, sg->offsets.p, (sg->n_sg + 1) * 8}, {hashes, sg->hashes.p, sg->n_out * 8},
            {edge_offsets, sg->ie_offsets.p, (sg->n_sg + 1) * 8}, {edges, sg->ie_edges.p, sg->n_ie * sizeof(sw_edge)},
            {used_mask, sg->used.p, sg->n_nodes}, {used_hashes, sg->used_hashes.p, sg->n_out * 8}};
        for (auto &x : c)
            if (x.dst && x.bytes) SW_HIP(hipMemcpy(x.dst, x.src, x.bytes, hipMemcpyDeviceToHost));
    });
}

int sw_subgraphs_stats(const sw_subgraphs *sg, uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (counters) memcpy(counters, sg->counters, sizeof sg->counters);
        if (ms) memcpy(ms, sg->ms, sizeof sg->ms);
    });
}

void sw_subgraphs_free(sw_subgraphs *sg)
{
    delete sg;
}

int sw_index_filter_kmers_sg(const sw_index *ix, const sw_index *nodes_from, const sw_subgraphs *sg, sw_index **out)
{
    return guarded([&] {
        const sw_index *nf = nodes_from ? nodes_from : ix;
        require_device(ix->device, "the index");
        if (nf->device != ix->device || sg->device != ix->device)
            raise(SW_ERR_VALUE, "the index, nodes_from and the subgraphs live on different devices (%d, %d, %d)", ix->device, nf->device, sg->device);
        std::unique_ptr<sw_index> o(new sw_index);
        o->device = ix->device;
        uint64_t nk = 0, nn = 0;
        device_filter_kmers(ix->kmers.p, ix->n_kmers, nf->nodes.p, nf->n_nodes, sg->used_hashes.p, sg->n_out, 0, o->kmers, o->nodes, &nk, &nn);
        o->n_kmers = nk;
        o->n_nodes = nn;
        o->n_edges = 0;
        o->edges.alloc(0);
        *out = o.release();
    });
}

}  // extern "C"
