// markers.hip -- markers._get_cks' per-subgraph work (src/seqwin/markers.py:95-300, 356-426) on the device: where every subgraph
// lies in every assembly (ConnectedKmers.__get_loc) and which k-mer ordering represents it (__get_rep_order), with the
// reference's result value for value.
//
// The kept index is sorted already: nodes ascending by hash, the occurrences of a node strictly ascending by (record_idx, pos).
// So nothing is sorted globally.  A PAIR is (subgraph, assembly); its items are the occurrences of the subgraph's nodes whose
// record lies in the assembly's record range, found by two binary searches per node.
//   1. k_count   one thread per pair: the number of its items.  Scans give every non-empty pair its row, in (subgraph, assembly)
//                order -- the order of the reference's `loc` -- and room for its k-mer ordering.
//   2. k_loc     one wave per row: gather the items, sort them by (record, pos) with the node's rank as payload (LDS; a pair
//                above the LDS bound sorts in an HBM scratch instead), cut the runs of consecutive minimizers with integer
//                arithmetic (2 * (pos - prev) > 3 * w is pandas' diff > 1.5 * w), keep the largest run, the earliest on ties.
//   3. k_vote    one workgroup per subgraph over its target rows (a prefix of its rows): fingerprint every ordering and its
//                reverse, sort the fingerprints, and settle equality EXACTLY, element by element, against the earlier rows of the
//                same fingerprint -- a fingerprint proposes, it never decides.  Orderings are compared as rank sequences: a
//                node's rank in the hash-sorted nodes orders as its hash.
// Both routes of include/seqwin_hip.h (the resident one and the one on host arrays) run this core.
#include <cstring>  // rocprim's texture iterator needs ::memset declared first
#include <memory>

#include <rocprim/rocprim.hpp>

#include "device.hpp"

namespace sw {
namespace {

constexpr int MK_WAVE = 64;
constexpr int MK_TPB = 256;
// LDS bounds.  A CU has 160 KiB of LDS and holds at most 32 waves.  k_loc runs one-wave workgroups: 5 KiB each keeps all 32
// resident; 384 items of 12 B (key + rank) are 4.5 KiB.  k_vote runs 4-wave workgroups, 8 per CU at 20 KiB each; 1536 rows of
// 12 B (fingerprint + row) are 18 KiB, 22 KiB with the reduction's arrays: 7 workgroups per CU.
constexpr uint32_t MK_LOC_CAP = 384;
constexpr uint32_t MK_VOTE_CAP = 1536;
constexpr uint32_t MK_NONE = 0xFFFFFFFFu;
constexpr uint32_t FLAG_SINGLE = 1, FLAG_DUP = 2, FLAG_NO_TARGET = 4;

inline unsigned mk_blocks(uint64_t n) { return (unsigned)((n + MK_TPB - 1) / MK_TPB); }

// first occurrence in [lo, hi) whose record is >= rec
__device__ inline uint64_t lb_rec(const sw_kmer *km, uint64_t lo, uint64_t hi, uint32_t rec)
{
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (km[mid].record_idx < rec) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Sorting network over n (key, value) pairs ascending by (key, value), by nt threads of one workgroup (thread t).  The bitonic
// merge in its all-ascending form -- the first step of a merge mirrors (i ^ (k - 1)), the rest halve --: every comparator puts
// the smaller pair at the lower index, so the places from n up to the next power of two act as +infinity without being stored.
__device__ inline void cmpx(uint64_t *k, uint32_t *v, uint32_t i, uint32_t j)
{
    const uint64_t a = k[i], b = k[j];
    const uint32_t x = v[i], y = v[j];
    if (a > b || (a == b && x > y)) { k[i] = b; k[j] = a; v[i] = y; v[j] = x; }
}
__device__ void sort_pairs(uint64_t *k, uint32_t *v, uint32_t n, uint32_t t, uint32_t nt)
{
    for (uint64_t kk = 2; (kk >> 1) < n; kk <<= 1) {
        for (uint32_t i = t; i < n; i += nt) {
            const uint64_t j = i ^ (kk - 1);
            if (j > i && j < n) cmpx(k, v, i, (uint32_t)j);
        }
        __syncthreads();
        for (uint32_t d = (uint32_t)(kk >> 2); d; d >>= 1) {
            for (uint32_t i = t; i < n; i += nt) {
                const uint32_t j = i ^ d;
                if (j > i && j < n) cmpx(k, v, i, j);
            }
            __syncthreads();
        }
    }
}

struct Core {   // the kept index and the subgraphs, on the device
    const sw_kmer *kmers;
    const sw_node *nodes;
    const uint64_t *sg_off;    // [n_sg + 1]
    const uint32_t *sg_rank;   // [sg_off[n_sg]] ranks of the subgraphs' nodes in `nodes`
    const uint32_t *ro;        // [n_asm + 1]
    uint64_t n_asm, n_sg;
};

// ---- 1. items per pair ----------------------------------------------------------------------------------------------------
__global__ void k_count(Core g, uint64_t n_pairs, uint32_t *cnt)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const uint64_t s = p / g.n_asm, a = p - s * g.n_asm;
    const uint32_t r0 = g.ro[a], r1 = g.ro[a + 1];
    uint32_t c = 0;
    if (r1 > r0)
        for (uint64_t j = g.sg_off[s]; j < g.sg_off[s + 1]; ++j) {
            const sw_node *nd = g.nodes + g.sg_rank[j];
            const uint64_t x = lb_rec(g.kmers, nd->start, nd->stop, r0), y = lb_rec(g.kmers, x, nd->stop, r1);
            c += (uint32_t)(y - x);
        }
    cnt[p] = c;
}

struct CntAt {
    const uint32_t *c;
    uint64_t n;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return i < n ? c[i] : 0; }
};
struct NonZeroAt {
    const uint32_t *c;
    uint64_t n;
    __host__ __device__ uint32_t operator()(uint64_t i) const { return i < n && c[i] ? 1u : 0u; }
};
struct SpillAt {
    const uint32_t *c;
    uint64_t n;
    uint32_t cap;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return i < n && c[i] > cap ? c[i] : 0; }
};
struct RowLenAt {
    const sw_marker_row *rows;
    uint64_t n;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return i < n ? rows[i].n_kmers : 0; }
};
struct RepLenAt {
    const sw_marker_rep *reps;
    uint64_t n;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return i < n ? reps[i].row.n_kmers : 0; }
};

// out[i] = sum of in[0, i) for i in [0, n]
template <class InIt, class T>
void scan_exclusive(InIt in, T *out, size_t n, hipStream_t stream)
{
    size_t tmp_bytes = 0;
    SW_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, in, out, T(0), n + 1, rocprim::plus<T>(), stream));
    DevArray<unsigned char> tmp(tmp_bytes);
    SW_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, in, out, T(0), n + 1, rocprim::plus<T>(), stream));
    SW_HIP(hipStreamSynchronize(stream));   // (tmp is released under the null stream: ordered anyway)
}

__global__ void k_row_list(const uint32_t *cnt, const uint32_t *rowi, uint64_t n_pairs, uint32_t *row_pair, uint32_t *row_cnt)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs || cnt[p] == 0) return;
    row_pair[rowi[p]] = (uint32_t)p;
    row_cnt[rowi[p]] = cnt[p];
}

// first row and number of target rows of every subgraph (targets are the assemblies below n_tar: a prefix of its rows)
__global__ void k_sg_rows(const uint32_t *rowi, uint64_t n_asm, uint64_t n_tar, uint64_t n_sg, uint64_t *row_off, uint32_t *tar_rows)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_sg) return;
    row_off[s] = rowi[s * n_asm];
    if (s < n_sg) tar_rows[s] = rowi[s * n_asm + n_tar] - rowi[s * n_asm];
}

// ---- 2. one row, one wave -------------------------------------------------------------------------------------------------
struct LocOut {
    const uint32_t *row_pair, *row_cnt;
    const uint64_t *seq_off;     // [n_rows + 1] room of every row's ordering in seq (its item count: an upper bound)
    const uint64_t *spill_off;   // [n_rows + 1] place of a row above the LDS bound in the scratch
    uint64_t *sk;                // scratch keys / ranks
    uint32_t *sr;
    sw_marker_row *rows;
    uint32_t *seq;               // rank sequences
    unsigned long long *stats;   // [0] spilled pairs, [1] largest pair
    uint32_t cap;                // LDS bound (SEQWIN_AMD_LOC_LDS_CAP lowers it)
    uint32_t kmerlen;
    uint64_t w3;                 // 3 * windowsize (saturated)
};

__device__ inline bool new_run(uint64_t prev, uint64_t cur, uint64_t w3)
{
    return (prev >> 32) != (cur >> 32) || 2 * ((cur & 0xFFFFFFFFull) - (prev & 0xFFFFFFFFull)) > w3;
}

__global__ void __launch_bounds__(MK_WAVE) k_loc(Core g, LocOut o)
{
    __shared__ uint64_t lk[MK_LOC_CAP];
    __shared__ uint32_t lr[MK_LOC_CAP];
    const uint32_t lane = threadIdx.x;
    const uint64_t r = blockIdx.x;
    const uint32_t p = o.row_pair[r], n = o.row_cnt[r];
    const uint64_t s = p / g.n_asm, a = p - s * g.n_asm;
    const uint32_t r0 = g.ro[a], r1 = g.ro[a + 1];
    const bool spill = n > o.cap;
    uint64_t *keys = spill ? o.sk + o.spill_off[r] : lk;
    uint32_t *rk = spill ? o.sr + o.spill_off[r] : lr;
    // gather: a lane per node, the items of the nodes one after the other
    uint32_t base = 0;
    const uint64_t j1 = g.sg_off[s + 1];
    for (uint64_t j0 = g.sg_off[s]; j0 < j1; j0 += MK_WAVE) {
        const uint64_t j = j0 + lane;
        uint64_t x = 0, y = 0;
        uint32_t rank = 0;
        if (j < j1) {
            rank = g.sg_rank[j];
            const sw_node *nd = g.nodes + rank;
            x = lb_rec(g.kmers, nd->start, nd->stop, r0);
            y = lb_rec(g.kmers, x, nd->stop, r1);
        }
        const uint32_t c = (uint32_t)(y - x);
        uint32_t inc = c;
        for (int d = 1; d < MK_WAVE; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, MK_WAVE);
            if ((int)lane >= d) inc += up;
        }
        uint32_t at = base + inc - c;
        for (uint64_t i = x; i < y; ++i, ++at)
            if (at < n) {   // (the count is the same search: always true)
                keys[at] = (uint64_t)g.kmers[i].record_idx << 32 | g.kmers[i].pos;
                rk[at] = rank;
            }
        base += __shfl(inc, MK_WAVE - 1, MK_WAVE);
    }
    __syncthreads();
    sort_pairs(keys, rk, n, lane, MK_WAVE);
    // runs: the start of the run every item lies in (a running maximum over the run starts), candidates at the run ends
    uint32_t carry = 0, n_runs = 0, best_len = 0, best_start = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += MK_WAVE) {
        const uint32_t i = i0 + lane;
        const bool valid = i < n;
        const uint64_t key = valid ? keys[i] : 0;
        const bool flag = valid && (i == 0 || new_run(keys[i - 1], key, o.w3));
        const bool end = valid && (i == n - 1 || new_run(key, keys[i + 1], o.w3));
        uint32_t st = flag ? i : 0;
        for (int d = 1; d < MK_WAVE; d <<= 1) {
            const uint32_t up = __shfl_up(st, d, MK_WAVE);
            if ((int)lane >= d && up > st) st = up;
        }
        if (carry > st) st = carry;
        if (end && i - st + 1 > best_len) { best_len = i - st + 1; best_start = st; }
        n_runs += (uint32_t)__popcll(__ballot(flag));
        carry = __shfl(st, MK_WAVE - 1, MK_WAVE);
    }
    for (int d = MK_WAVE / 2; d; d >>= 1) {
        const uint32_t ol = __shfl_xor(best_len, d, MK_WAVE), os = __shfl_xor(best_start, d, MK_WAVE);
        if (ol > best_len || (ol == best_len && os < best_start)) { best_len = ol; best_start = os; }
    }
    if (n == 0) return;   // (no such row)
    uint32_t *dst = o.seq + o.seq_off[r];
    for (uint32_t i = lane; i < best_len; i += MK_WAVE) dst[i] = rk[best_start + i];
    if (lane == 0) {
        const uint64_t first = keys[best_start], last = keys[best_start + best_len - 1];
        sw_marker_row row;
        row.assembly_idx = (uint32_t)a;
        row.record_idx = (uint32_t)(first >> 32) - r0;
        row.start = (uint32_t)first;
        row.stop = (uint32_t)last + o.kmerlen;   // uint32, as the reference's column stays
        row.n_kmers = best_len;
        row.n_repeats = n_runs;
        o.rows[r] = row;
        if (spill) atomicAdd(&o.stats[0], 1ull);
        atomicMax(&o.stats[1], (unsigned long long)n);
    }
}

// ---- 3. the vote, one workgroup per subgraph -------------------------------------------------------------------------------
struct Vote {
    const uint64_t *row_off;     // [n_sg + 1]
    const uint32_t *tar_rows;    // [n_sg]
    const sw_marker_row *rows;
    const uint64_t *seq_off;
    const uint32_t *seq;
    uint64_t *rfp;               // per row: fingerprint of the reversed ordering
    uint32_t *lead;              // per row: the first row of the subgraph with the same ordering (local index)
    uint32_t *cnt;               // per row: rows with a leader's ordering (zeroed)
    uint8_t *revless;            // per row: the reversed ordering is the smaller one
    uint64_t *vk;                // scratch of subgraphs above the LDS bound: fingerprints / rows, indexed by row
    uint32_t *vi;
    sw_marker_rep *reps;
    uint32_t *rep_row;           // [n_sg] row holding the representative ordering
    unsigned long long *stats;   // [2] vote spills
    uint32_t cap;                // LDS bound
    uint64_t fp_mask;            // fingerprint bits in use (SEQWIN_AMD_LOC_FP_BITS narrows them: collisions on small inputs)
};

__device__ inline bool seq_equal(const uint32_t *a, uint32_t la, const uint32_t *b, uint32_t lb)
{
    if (la != lb) return false;
    for (uint32_t i = 0; i < la; ++i)
        if (a[i] != b[i]) return false;
    return true;
}
__device__ inline bool seq_equal_rev(const uint32_t *a, uint32_t la, const uint32_t *b, uint32_t lb)
{
    if (la != lb) return false;
    for (uint32_t i = 0; i < la; ++i)
        if (a[i] != b[la - 1 - i]) return false;
    return true;
}
__device__ inline uint32_t lower_bound_fp(const uint64_t *k, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (k[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(MK_TPB) k_vote(Vote v)
{
    __shared__ uint64_t lk[MK_VOTE_CAP];
    __shared__ uint32_t li[MK_VOTE_CAP];
    __shared__ unsigned long long red_score[MK_TPB];
    __shared__ uint32_t red_j[MK_TPB], red_p[MK_TPB];
    __shared__ uint32_t s_dup;
    const uint32_t t = threadIdx.x;
    const uint64_t s = blockIdx.x;
    const uint64_t R0 = v.row_off[s];
    const uint32_t T = v.tar_rows[s];
    if (T == 0) {
        if (t == 0) {
            sw_marker_rep rep;
            memset(&rep, 0, sizeof rep);
            rep.flags = FLAG_NO_TARGET;
            v.reps[s] = rep;
            v.rep_row[s] = MK_NONE;
        }
        return;
    }
    const bool spill = T > v.cap;
    uint64_t *fk = spill ? v.vk + R0 : lk;
    uint32_t *fi = spill ? v.vi + R0 : li;
    if (t == 0) {
        s_dup = 0;
        if (spill) atomicAdd(&v.stats[2], 1ull);
    }
    // fingerprints of every ordering and of its reverse; which of the two is the smaller
    for (uint32_t j = t; j < T; j += MK_TPB) {
        const uint32_t L = v.rows[R0 + j].n_kmers;
        const uint32_t *q = v.seq + v.seq_off[R0 + j];
        uint64_t hf = CK_G ^ L, hr = CK_G ^ L;
        for (uint32_t i = 0; i < L; ++i) {
            hf = mix64(hf + q[i] + CK_K1);
            hr = mix64(hr + q[L - 1 - i] + CK_K1);
        }
        uint8_t less = 0;
        for (uint32_t i = 0; i < L; ++i) {
            const uint32_t x = q[i], y = q[L - 1 - i];
            if (x != y) { less = y < x; break; }
        }
        fk[j] = hf & v.fp_mask;
        fi[j] = j;
        v.rfp[R0 + j] = hr & v.fp_mask;
        v.revless[R0 + j] = less;
    }
    __syncthreads();
    sort_pairs(fk, fi, T, t, MK_TPB);
    // leaders: the first earlier row of the same fingerprint that is equal element for element
    for (uint32_t q = t; q < T; q += MK_TPB) {
        const uint32_t j = fi[q];
        const uint32_t L = v.rows[R0 + j].n_kmers;
        const uint32_t *sj = v.seq + v.seq_off[R0 + j];
        uint32_t leader = j;
        for (uint32_t i = lower_bound_fp(fk, T, fk[q]); i < q; ++i) {
            const uint32_t j2 = fi[i];
            if (seq_equal(sj, L, v.seq + v.seq_off[R0 + j2], v.rows[R0 + j2].n_kmers)) { leader = j2; break; }
        }
        v.lead[R0 + j] = leader;
        atomicAdd(&v.cnt[R0 + leader], 1u);
    }
    __syncthreads();
    // canonical groups: a leader and the leader holding its reverse, if any.  The group is scored at the earlier of the two
    // (its first appearance while walking the orderings in row order).
    unsigned long long best = 0;
    uint32_t best_j = MK_NONE, best_p = MK_NONE;
    for (uint32_t j = t; j < T; j += MK_TPB) {
        if (v.lead[R0 + j] != j) continue;
        const uint32_t L = v.rows[R0 + j].n_kmers;
        const uint32_t *sj = v.seq + v.seq_off[R0 + j];
        uint32_t partner = MK_NONE;
        const uint64_t rf = v.rfp[R0 + j];
        for (uint32_t i = lower_bound_fp(fk, T, rf); i < T && fk[i] == rf; ++i) {
            const uint32_t j2 = fi[i];
            if (v.lead[R0 + j2] != j2) continue;
            if (seq_equal_rev(sj, L, v.seq + v.seq_off[R0 + j2], v.rows[R0 + j2].n_kmers)) { partner = j2; break; }
        }
        if (partner == j) partner = MK_NONE;   // a palindrome is its own reverse: one key, counted once
        if (partner != MK_NONE && partner < j) continue;
        const unsigned long long cc = (unsigned long long)atomicAdd(&v.cnt[R0 + j], 0u) +
                                      (partner != MK_NONE ? atomicAdd(&v.cnt[R0 + partner], 0u) : 0u);
        const unsigned long long score = (unsigned long long)L * cc;
        if (best_j == MK_NONE || score > best) { best = score; best_j = j; best_p = partner; }   // (j ascends: the first stays on ties)
    }
    red_score[t] = best;
    red_j[t] = best_j;
    red_p[t] = best_p;
    __syncthreads();
    for (uint32_t d = MK_TPB / 2; d; d >>= 1) {
        if (t < d) {
            const uint32_t oj = red_j[t + d];
            if (oj != MK_NONE && (red_j[t] == MK_NONE || red_score[t + d] > red_score[t] || (red_score[t + d] == red_score[t] && oj < red_j[t]))) {
                red_score[t] = red_score[t + d];
                red_j[t] = oj;
                red_p[t] = red_p[t + d];
            }
        }
        __syncthreads();
    }
    const uint32_t j = red_j[0], pj = red_p[0];
    const uint32_t cj = atomicAdd(&v.cnt[R0 + j], 0u), cp = pj != MK_NONE ? atomicAdd(&v.cnt[R0 + pj], 0u) : 0u;
    uint32_t rep = j;
    if (pj != MK_NONE) {
        // the canonical ordering is j's unless its reverse is smaller; it stands if it is at least as common as the other
        if (!v.revless[R0 + j]) rep = cj >= cp ? j : pj;
        else rep = cp >= cj ? pj : j;
    }
    const sw_marker_row row = v.rows[R0 + rep];
    const uint32_t *sr = v.seq + v.seq_off[R0 + rep];
    for (uint32_t i = t; i < row.n_kmers; i += MK_TPB) {
        const uint32_t x = sr[i];
        bool dup = false;
        for (uint32_t i2 = 0; i2 < i && !dup; ++i2) dup = sr[i2] == x;
        if (dup) s_dup = 1;
    }
    __syncthreads();
    if (t == 0) {
        sw_marker_rep out;
        out.row = row;
        out.n_rep = cj + cp;
        out.flags = (row.n_kmers == 1 ? FLAG_SINGLE : 0) | (s_dup ? FLAG_DUP : 0);
        v.reps[s] = out;
        v.rep_row[s] = (uint32_t)rep;
    }
}

// ---- results --------------------------------------------------------------------------------------------------------------
// the hashes of the representative orderings (one wave per subgraph)
__global__ void __launch_bounds__(MK_WAVE) k_rep_hashes(const sw_marker_rep *reps, const uint32_t *rep_row, const uint64_t *row_off,
                                                        const uint64_t *seq_off, const uint32_t *seq, const sw_node *nodes,
                                                        const uint64_t *rep_off, uint64_t *out)
{
    const uint64_t s = blockIdx.x;
    if (rep_row[s] == MK_NONE) return;
    const uint32_t *q = seq + seq_off[row_off[s] + rep_row[s]];
    const uint32_t L = reps[s].row.n_kmers;
    for (uint32_t i = threadIdx.x; i < L; i += MK_WAVE) out[rep_off[s] + i] = nodes[q[i]].hash;
}

// the hashes of every row's ordering (one wave per row)
__global__ void __launch_bounds__(MK_WAVE) k_row_hashes(const sw_marker_row *rows, const uint64_t *seq_off, const uint32_t *seq,
                                                        const sw_node *nodes, const uint64_t *kmer_off, uint64_t *out)
{
    const uint64_t r = blockIdx.x;
    const uint32_t *q = seq + seq_off[r];
    const uint32_t L = rows[r].n_kmers;
    for (uint32_t i = threadIdx.x; i < L; i += MK_WAVE) out[kmer_off[r] + i] = nodes[q[i]].hash;
}

// ranks of the subgraphs' hashes in the kept nodes (resident route); a hash that is no kept node sets *err
__global__ void k_sg_ranks(const uint64_t *hashes, uint64_t n, const sw_node *nodes, uint64_t n_nodes, uint32_t *rank, unsigned int *err)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = hashes[i];
    uint64_t lo = 0, hi = n_nodes;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (nodes[mid].hash < h) lo = mid + 1; else hi = mid;
    }
    if (lo >= n_nodes || nodes[lo].hash != h) {
        atomicOr(err, 1u);
        lo = 0;
    }
    rank[i] = (uint32_t)lo;
}

// the records the index holds: occurrences ascend by record inside a node, so its first and last one bound them;
// a node range outside the occurrences sets *err
__global__ void k_rec_range(const sw_kmer *kmers, uint64_t n_kmers, const sw_node *nodes, uint64_t n_nodes, uint32_t *lo, uint32_t *hi,
                            unsigned int *err)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const uint64_t a = nodes[i].start, b = nodes[i].stop;
    if (a > b || b > n_kmers) {
        atomicOr(err, 1u);
        return;
    }
    if (a == b) return;
    atomicMin(lo, kmers[a].record_idx);
    atomicMax(hi, kmers[b - 1].record_idx);
}

}  // namespace
}  // namespace sw

namespace sw {
namespace {

void check_args(const uint32_t *ro, uint64_t n_asm, uint64_t n_tar, uint64_t windowsize)
{
    if (!ro) raise(SW_ERR_VALUE, "record_offsets is NULL");
    if (n_asm >= 0xFFFFFFFFull) raise(SW_ERR_VALUE, "markers: %llu assemblies exceed 32-bit indices", (unsigned long long)n_asm);
    for (uint64_t a = 0; a < n_asm; ++a)
        if (ro[a] > ro[a + 1]) raise(SW_ERR_VALUE, "record_offsets must be non-decreasing (assembly %llu)", (unsigned long long)a);
    if (n_tar > n_asm) raise(SW_ERR_VALUE, "n_tar = %llu exceeds the %llu assemblies", (unsigned long long)n_tar, (unsigned long long)n_asm);
    if (windowsize < 1) raise(SW_ERR_VALUE, "windowsize must be >= 1");
}

// The device core of both routes.  kmers / nodes: the kept index; sg_off / sg_rank: the subgraphs as CSR of node ranks.
void run_markers(const sw_kmer *kmers, uint64_t n_kmers, const sw_node *nodes, uint64_t n_nodes, const uint64_t *sg_off,
                 const uint32_t *sg_rank, uint64_t n_sg, const uint32_t *ro_host, uint64_t n_asm, uint64_t n_tar, uint64_t kmerlen,
                 uint64_t windowsize, int keep_rows, sw_markers &o)
{
    hipStream_t stream = 0;
    if (n_kmers >= 0xFFFFFFFEull) raise_occ_cap(n_kmers, "marker locations");
    if (n_nodes >= MK_NONE) raise(SW_ERR_VALUE, "markers: %llu nodes exceed the 32-bit ranks", (unsigned long long)n_nodes);
    const uint64_t n_pairs = n_sg * n_asm;
    if (n_sg && n_pairs / n_sg != n_asm) raise(SW_ERR_VALUE, "markers: subgraphs x assemblies overflows");
    if (n_pairs >= 0xFFFFFFFFull)
        raise(SW_ERR_VALUE, "markers: %llu subgraphs x %llu assemblies exceed the 32-bit pair index", (unsigned long long)n_sg,
              (unsigned long long)n_asm);
    Event e0, e1, e2, e3, e4;
    SW_HIP(hipEventRecord(e0, stream));
    // the record table covers the records of the index
    DevArray<uint32_t> d_ro(n_asm + 1);
    SW_HIP(hipMemcpyAsync(d_ro.p, ro_host, (n_asm + 1) * 4, hipMemcpyHostToDevice, stream));
    {
        DevArray<uint32_t> range(2);
        DevArray<unsigned int> err(1);
        const uint32_t init[2] = {0xFFFFFFFFu, 0u};
        SW_HIP(hipMemcpyAsync(range.p, init, 8, hipMemcpyHostToDevice, stream));
        SW_HIP(hipMemsetAsync(err.p, 0, 4, stream));
        if (n_nodes)
            hipLaunchKernelGGL(k_rec_range, dim3(mk_blocks(n_nodes)), dim3(MK_TPB), 0, stream, kmers, n_kmers, nodes, n_nodes, range.p,
                               range.p + 1, err.p);
        SW_HIP(hipGetLastError());
        uint32_t h[2];
        unsigned int e = 0;
        SW_HIP(hipMemcpyAsync(h, range.p, 8, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipMemcpyAsync(&e, err.p, 4, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
        if (e) raise(SW_ERR_VALUE, "markers: a node's [start, stop) lies outside the %llu occurrences", (unsigned long long)n_kmers);
        if (h[0] <= h[1] && (h[0] < ro_host[0] || h[1] >= ro_host[n_asm]))
            raise(SW_ERR_VALUE, "record_offsets [%u, %u) do not cover the index's records %u .. %u", ro_host[0], ro_host[n_asm], h[0], h[1]);
    }
    const uint32_t loc_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(env_u64(SW_TEST_GETENV("SEQWIN_AMD_LOC_LDS_CAP"), MK_LOC_CAP), 1), MK_LOC_CAP);
    const uint32_t vote_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(env_u64(SW_TEST_GETENV("SEQWIN_AMD_LOC_VOTE_CAP"), MK_VOTE_CAP), 1), MK_VOTE_CAP);
    const uint64_t fp_bits = std::min<uint64_t>(env_u64(SW_TEST_GETENV("SEQWIN_AMD_LOC_FP_BITS"), 64), 64);
    const uint64_t fp_mask = fp_bits >= 64 ? ~0ull : (1ull << fp_bits) - 1;
    Core g{kmers, nodes, sg_off, sg_rank, d_ro.p, n_asm, n_sg};

    // ---- 1. items per pair, rows ----
    DevArray<uint32_t> cnt(n_pairs), rowi(n_pairs + 1);
    if (n_pairs) hipLaunchKernelGGL(k_count, dim3(mk_blocks(n_pairs)), dim3(MK_TPB), 0, stream, g, n_pairs, cnt.p);
    SW_HIP(hipGetLastError());
    scan_exclusive(rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), NonZeroAt{cnt.p, n_pairs}), rowi.p, n_pairs, stream);
    uint32_t n_rows32 = 0;
    SW_HIP(hipMemcpyAsync(&n_rows32, rowi.p + n_pairs, 4, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    const uint64_t n_rows = n_rows32;
    if (n_rows >= (1ull << 31)) raise(SW_ERR_VALUE, "markers: %llu rows exceed one launch", (unsigned long long)n_rows);
    DevArray<uint32_t> row_pair(n_rows), row_cnt(n_rows), tar_rows(n_sg);
    DevArray<uint64_t> seq_off(n_rows + 1), spill_off(n_rows + 1);
    o.row_off.alloc(n_sg + 1);
    if (n_pairs) hipLaunchKernelGGL(k_row_list, dim3(mk_blocks(n_pairs)), dim3(MK_TPB), 0, stream, cnt.p, rowi.p, n_pairs, row_pair.p, row_cnt.p);
    if (n_asm)
        hipLaunchKernelGGL(k_sg_rows, dim3(mk_blocks(n_sg + 1)), dim3(MK_TPB), 0, stream, rowi.p, n_asm, n_tar, n_sg, o.row_off.p, tar_rows.p);
    else {
        SW_HIP(hipMemsetAsync(o.row_off.p, 0, (n_sg + 1) * 8, stream));
        if (n_sg) SW_HIP(hipMemsetAsync(tar_rows.p, 0, n_sg * 4, stream));
    }
    SW_HIP(hipGetLastError());
    cnt.release();
    rowi.release();
    scan_exclusive(rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), CntAt{row_cnt.p, n_rows}), seq_off.p, n_rows, stream);
    scan_exclusive(rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), SpillAt{row_cnt.p, n_rows, loc_cap}),
                   spill_off.p, n_rows, stream);
    uint64_t n_items = 0, n_spill_items = 0;
    SW_HIP(hipMemcpyAsync(&n_items, seq_off.p + n_rows, 8, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipMemcpyAsync(&n_spill_items, spill_off.p + n_rows, 8, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    SW_HIP(hipEventRecord(e1, stream));

    // ---- 2. the rows ----
    DevArray<uint32_t> seq(n_items), sr(n_spill_items);
    DevArray<uint64_t> sk(n_spill_items);
    DevArray<unsigned long long> stats(3);
    SW_HIP(hipMemsetAsync(stats.p, 0, 24, stream));
    o.rows.alloc(n_rows);
    const uint64_t w3 = windowsize > (1ull << 34) ? ~0ull : 3 * windowsize;   // 2 * (a difference of two uint32) stays below 2^33
    LocOut lo{row_pair.p, row_cnt.p, seq_off.p, spill_off.p, sk.p, sr.p, o.rows.p, seq.p, stats.p, loc_cap, (uint32_t)kmerlen, w3};
    if (n_rows) hipLaunchKernelGGL(k_loc, dim3((unsigned)n_rows), dim3(MK_WAVE), 0, stream, g, lo);
    SW_HIP(hipGetLastError());
    SW_HIP(hipEventRecord(e2, stream));

    // ---- 3. the vote ----
    const bool vote_scratch = n_tar > vote_cap;
    DevArray<uint64_t> rfp(n_rows), vk(vote_scratch ? n_rows : 0);
    DevArray<uint32_t> lead(n_rows), vcnt(n_rows), vi(vote_scratch ? n_rows : 0), rep_row(n_sg);
    DevArray<uint8_t> revless(n_rows);
    if (n_rows) SW_HIP(hipMemsetAsync(vcnt.p, 0, n_rows * 4, stream));
    o.reps.alloc(n_sg);
    Vote v{o.row_off.p, tar_rows.p, o.rows.p, seq_off.p, seq.p, rfp.p, lead.p, vcnt.p, revless.p, vk.p, vi.p, o.reps.p, rep_row.p, stats.p,
           vote_cap, fp_mask};
    if (n_sg) hipLaunchKernelGGL(k_vote, dim3((unsigned)n_sg), dim3(MK_TPB), 0, stream, v);
    SW_HIP(hipGetLastError());
    SW_HIP(hipEventRecord(e3, stream));

    // ---- results ----
    o.rep_off.alloc(n_sg + 1);
    scan_exclusive(rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), RepLenAt{o.reps.p, n_sg}), o.rep_off.p, n_sg, stream);
    SW_HIP(hipMemcpyAsync(&o.n_rep_kmers, o.rep_off.p + n_sg, 8, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    o.rep_hashes.alloc(o.n_rep_kmers);
    if (n_sg)
        hipLaunchKernelGGL(k_rep_hashes, dim3((unsigned)n_sg), dim3(MK_WAVE), 0, stream, o.reps.p, rep_row.p, o.row_off.p, seq_off.p, seq.p, nodes,
                           o.rep_off.p, o.rep_hashes.p);
    SW_HIP(hipGetLastError());
    o.n_sg = n_sg;
    o.n_rows = n_rows;
    o.keep_rows = keep_rows;
    o.record_offsets.assign(ro_host, ro_host + n_asm + 1);
    if (keep_rows) {
        o.kmer_off.alloc(n_rows + 1);
        scan_exclusive(rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), RowLenAt{o.rows.p, n_rows}), o.kmer_off.p,
                       n_rows, stream);
        SW_HIP(hipMemcpyAsync(&o.n_row_kmers, o.kmer_off.p + n_rows, 8, hipMemcpyDeviceToHost, stream));
        SW_HIP(hipStreamSynchronize(stream));
        o.row_hashes.alloc(o.n_row_kmers);
        if (n_rows)
            hipLaunchKernelGGL(k_row_hashes, dim3((unsigned)n_rows), dim3(MK_WAVE), 0, stream, o.rows.p, seq_off.p, seq.p, nodes, o.kmer_off.p,
                               o.row_hashes.p);
        SW_HIP(hipGetLastError());
    }
    unsigned long long hs[3] = {};
    SW_HIP(hipMemcpyAsync(hs, stats.p, 24, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipEventRecord(e4, stream));
    SW_HIP(hipStreamSynchronize(stream));
    if (!keep_rows) {
        o.rows.release();
        o.row_off.release();
    }
    const uint64_t cn[4] = {n_rows, hs[0], hs[1], hs[2]};
    memcpy(o.counters, cn, sizeof cn);
    hipEvent_t ev[5] = {e0, e1, e2, e3, e4};
    for (int i = 0; i < 4; ++i) {
        float ms = 0;
        SW_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        o.ms[i] = ms;
    }
}

}  // namespace
}  // namespace sw

using namespace sw;

extern "C" {

int sw_index_marker_locs(const sw_index *kept, const sw_subgraphs *sg, const uint32_t *record_offsets, uint64_t n_assemblies, uint64_t n_tar,
                         uint64_t kmerlen, uint64_t windowsize, int keep_rows, sw_markers **out)
{
    return guarded([&] {
        if (!kept || !sg || !out) raise(SW_ERR_VALUE, "markers: a NULL handle");
        check_args(record_offsets, n_assemblies, n_tar, windowsize);
        require_device(kept->device, "the index");
        int sg_dev = 0;
        uint64_t n_sg = 0, n_out = 0;
        const uint64_t *offs = nullptr, *hashes = nullptr;
        subgraphs_csr(sg, &sg_dev, &n_sg, &n_out, &offs, &hashes);
        if (sg_dev != kept->device) raise(SW_ERR_VALUE, "the index and the subgraphs live on different devices (%d, %d)", kept->device, sg_dev);
        DevArray<uint32_t> rank(n_out);
        DevArray<unsigned int> err(1);
        SW_HIP(hipMemsetAsync(err.p, 0, 4, 0));
        if (n_out)
            hipLaunchKernelGGL(k_sg_ranks, dim3(mk_blocks(n_out)), dim3(MK_TPB), 0, 0, hashes, n_out, kept->nodes.p, kept->n_nodes, rank.p, err.p);
        SW_HIP(hipGetLastError());
        unsigned int e = 0;
        SW_HIP(hipMemcpy(&e, err.p, 4, hipMemcpyDeviceToHost));
        if (e) raise(SW_ERR_VALUE, "markers: a subgraph node is not among the index's nodes (pass the index of sw_index_filter_kmers_sg)");
        std::unique_ptr<sw_markers> o(new sw_markers);
        o->device = kept->device;
        run_markers(kept->kmers.p, kept->n_kmers, kept->nodes.p, kept->n_nodes, offs, rank.p, n_sg, record_offsets, n_assemblies, n_tar, kmerlen,
                    windowsize, keep_rows, *o);
        *out = o.release();
    });
}

int sw_marker_locs_from_arrays(const sw_kmer *kmers, uint64_t n_kmers, const sw_node *nodes, uint64_t n_nodes, const uint64_t *sg_offsets,
                               const uint64_t *sg_nodes, uint64_t n_sg, const uint32_t *record_offsets, uint64_t n_assemblies, uint64_t n_tar,
                               uint64_t kmerlen, uint64_t windowsize, int keep_rows, sw_markers **out)
{
    return guarded([&] {
        if (!out || !sg_offsets || (n_kmers && !kmers) || (n_nodes && !nodes)) raise(SW_ERR_VALUE, "markers: a NULL array");
        check_args(record_offsets, n_assemblies, n_tar, windowsize);
        if (n_nodes >= MK_NONE) raise(SW_ERR_VALUE, "markers: %llu nodes exceed the 32-bit ranks", (unsigned long long)n_nodes);
        for (uint64_t i = 0; i < n_nodes; ++i) {
            if (i && !(nodes[i - 1].hash < nodes[i].hash)) raise(SW_ERR_VALUE, "nodes must be strictly ascending by hash (node %llu)", (unsigned long long)i);
            if (nodes[i].start > nodes[i].stop || nodes[i].stop > n_kmers)
                raise(SW_ERR_VALUE, "node %llu: [start, stop) lies outside the %llu occurrences", (unsigned long long)i, (unsigned long long)n_kmers);
            for (uint64_t j = nodes[i].start + 1; j < nodes[i].stop; ++j) {
                const uint64_t a = (uint64_t)kmers[j - 1].record_idx << 32 | kmers[j - 1].pos, b = (uint64_t)kmers[j].record_idx << 32 | kmers[j].pos;
                if (!(a < b)) raise(SW_ERR_VALUE, "node %llu: occurrences must be strictly ascending by (record_idx, pos)", (unsigned long long)i);
            }
        }
        if (sg_offsets[0] != 0) raise(SW_ERR_VALUE, "sg_offsets must start at 0");
        for (uint64_t s = 0; s < n_sg; ++s)
            if (sg_offsets[s] > sg_offsets[s + 1]) raise(SW_ERR_VALUE, "sg_offsets must be non-decreasing (subgraph %llu)", (unsigned long long)s);
        const uint64_t n_out = sg_offsets[n_sg];
        if (n_out && !sg_nodes) raise(SW_ERR_VALUE, "markers: a NULL array");
        std::vector<uint32_t> rank(n_out);
        for (uint64_t i = 0; i < n_out; ++i) {
            if (sg_nodes[i] >= n_nodes) raise(SW_ERR_VALUE, "sg_nodes[%llu] = %llu is no node", (unsigned long long)i, (unsigned long long)sg_nodes[i]);
            rank[i] = (uint32_t)sg_nodes[i];
        }
        std::unique_ptr<sw_markers> o(new sw_markers);
        SW_HIP(hipGetDevice(&o->device));
        DevArray<sw_kmer> d_kmers(n_kmers);
        DevArray<sw_node> d_nodes(n_nodes);
        DevArray<uint64_t> d_off(n_sg + 1);
        DevArray<uint32_t> d_rank(n_out);
        if (n_kmers) SW_HIP(hipMemcpy(d_kmers.p, kmers, n_kmers * sizeof(sw_kmer), hipMemcpyHostToDevice));
        if (n_nodes) SW_HIP(hipMemcpy(d_nodes.p, nodes, n_nodes * sizeof(sw_node), hipMemcpyHostToDevice));
        SW_HIP(hipMemcpy(d_off.p, sg_offsets, (n_sg + 1) * 8, hipMemcpyHostToDevice));
        if (n_out) SW_HIP(hipMemcpy(d_rank.p, rank.data(), n_out * 4, hipMemcpyHostToDevice));
        run_markers(d_kmers.p, n_kmers, d_nodes.p, n_nodes, d_off.p, d_rank.p, n_sg, record_offsets, n_assemblies, n_tar, kmerlen, windowsize,
                    keep_rows, *o);
        *out = o.release();
    });
}

int sw_markers_sizes(const sw_markers *m, uint64_t *n_sg, uint64_t *n_rep_kmers, uint64_t *n_rows, uint64_t *n_row_kmers)
{
    return guarded([&] {
        if (n_sg) *n_sg = m->n_sg;
        if (n_rep_kmers) *n_rep_kmers = m->n_rep_kmers;
        if (n_rows) *n_rows = m->n_rows;
        if (n_row_kmers) *n_row_kmers = m->n_row_kmers;
    });
}

int sw_markers_export(const sw_markers *m, sw_marker_rep *reps, uint64_t *rep_offsets, uint64_t *rep_hashes)
{
    return guarded([&] {
        require_device(m->device, "the markers");
        struct { void *dst; const void *src; uint64_t bytes; } c[3] = {{reps, m->reps.p, m->n_sg * sizeof(sw_marker_rep)},
                                                                       {rep_offsets, m->rep_off.p, (m->n_sg + 1) * 8},
                                                                       {rep_hashes, m->rep_hashes.p, m->n_rep_kmers * 8}};
        for (auto &x : c)
            if (x.dst && x.bytes) SW_HIP(hipMemcpy(x.dst, x.src, x.bytes, hipMemcpyDeviceToHost));
    });
}

int sw_markers_export_rows(const sw_markers *m, uint64_t *row_offsets, sw_marker_row *rows, uint64_t *kmer_offsets, uint64_t *row_hashes)
{
    return guarded([&] {
        if (!m->keep_rows) raise(SW_ERR_VALUE, "the rows were not kept (keep_rows = 0)");
        require_device(m->device, "the markers");
        struct { void *dst; const void *src; uint64_t bytes; } c[4] = {{row_offsets, m->row_off.p, (m->n_sg + 1) * 8},
                                                                       {rows, m->rows.p, m->n_rows * sizeof(sw_marker_row)},
                                                                       {kmer_offsets, m->kmer_off.p, (m->n_rows + 1) * 8},
                                                                       {row_hashes, m->row_hashes.p, m->n_row_kmers * 8}};
        for (auto &x : c)
            if (x.dst && x.bytes) SW_HIP(hipMemcpy(x.dst, x.src, x.bytes, hipMemcpyDeviceToHost));
    });
}

int sw_markers_stats(const sw_markers *m, uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (counters) memcpy(counters, m->counters, sizeof m->counters);
        if (ms) memcpy(ms, m->ms, sizeof m->ms);
    });
}

void sw_markers_free(sw_markers *m)
{
    delete m;
}

}  // extern "C"
