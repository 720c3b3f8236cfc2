// seqs.hip -- intervals of the resident 2-bit batch: their text, and exact edit distances between pairs of them.
//
// Replaces markers._fetch_cks_seq (src/seqwin/markers.py:428-471, over Assemblies.fetch_seq / _fetch_seq / load_fasta,
// assemblies.py:101-141, 282-297, utils.py:492-530: every FASTA file a representative lies in is read a second time) by a decode
// of the packed bases that are resident anyway, and adds a quantity the reference does not have: the Levenshtein distance between
// a representative and every located copy of its subgraph (DESIGN.md section 3.2c is the specification; tests/tools/seqs_host.py
// restates both).
//
//   k_iv_check    first interval with record >= n_records, start > stop or stop > rec_len (the lists may have been built on the device)
//   k_fetch       one wave per interval: a lane decodes one base per step from d_packed and stores one byte -- 64 consecutive bytes
//                 per store --; validity comes from the record's runs (searched once per wave; per lane only for an interval that is
//                 not inside one run, which is also what SW_SEQ_INEXACT says)
//   k_ed_classify the shorter side of a pair is the pattern; pairs are listed by the power of two >= their pattern blocks of 64 rows
//   k_ed          Myers' bit-vector recurrence (Hyyro's block form) over 64-row blocks: a group of g = 1, 2, ... 64 lanes holds one
//                 pair, lane b block b; at step t lane b does column t - b, and the column's base travels down the lanes together
//                 with the block's horizontal delta in one shuffle.  Block state (Pv, Mv) and the pattern's bit planes live in
//                 registers.  Both strands are advanced in the same step (two independent chains).  A pattern above ED_CAP blocks is
//                 cut into stripes of g blocks; the last lane of a stripe leaves its deltas in an HBM row that lane 0 of the next reads.
//   k_mk_*        the interval lists of a sw_markers: representatives, rows, and (representative, row) pairs
#include "seqs_core.hpp"

namespace sw {
namespace {

// ---- fetch ----------------------------------------------------------------------------------------------------------------------
// intervals [i0, i1) of the list, SQ_PER_WAVE at most per wave
__global__ __launch_bounds__(SQ_TPB) void k_fetch(RunTable t, const sw_interval *__restrict__ iv, const uint64_t *__restrict__ off, uint64_t i0,
                                                  uint64_t i1, char *__restrict__ blob, uint8_t *__restrict__ flags)
{
    const uint32_t lane = threadIdx.x % SQ_WAVE;
    const uint64_t waves = (uint64_t)gridDim.x * SQ_WPB;
    for (uint64_t i = i0 + (uint64_t)blockIdx.x * SQ_WPB + threadIdx.x / SQ_WAVE; i < i1; i += waves) {   // (uniform in the wave)
        const sw_interval v = iv[i];
        const uint32_t len = v.stop - v.start;
        const uint64_t o = off[i], base = t.rec_base[v.record] + v.start;
        const uint32_t q1 = t.rec_run_off[v.record + 1];
        const uint32_t qa = run_behind(t, t.rec_run_off[v.record], q1, v.start);
        // inside one valid run: runs are maximal, so this is "every base of the interval is valid"
        const bool whole = len == 0 || (qa < q1 && t.run_pos[qa] <= v.start && (uint64_t)t.run_pos[qa] + t.run_len[qa] >= v.stop);
        for (uint32_t b = lane; b < len; b += SQ_WAVE) {
            const uint64_t gp = base + b;
            const uint32_t code = (t.packed[gp >> 4] >> (2 * (uint32_t)(gp & 15))) & 3u;
            bool valid = whole;
            if (!whole) {
                const uint32_t p = v.start + b;
                uint32_t lo = qa, hi = q1;   // first run that starts behind p
                while (lo < hi) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (t.run_pos[mid] <= p) lo = mid + 1; else hi = mid;
                }
                valid = lo > qa && (uint64_t)t.run_pos[lo - 1] + t.run_len[lo - 1] > p;
            }
            blob[o + b] = valid ? (char)(0x54474341u >> (8 * code)) : 'N';   // "ACGT"
        }
        if (lane == 0) flags[i] = whole ? 0 : (uint8_t)SW_SEQ_INEXACT;
    }
}

struct IvLenAt {
    const sw_interval *iv;
    uint64_t n;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return i < n ? (uint64_t)(iv[i].stop - iv[i].start) : 0; }
};

// ---- edit distances -------------------------------------------------------------------------------------------------------------
struct EdArgs {
    RunTable t;
    const sw_interval *R, *S;
    const uint32_t *list;     // pair indices of this launch's class
    uint64_t count;           // entries of list
    uint32_t g;               // lanes per pair (a power of two <= 64)
    uint8_t *carry;           // striped route: one row of carry_stride bytes per group of the launch
    uint64_t carry_stride;    // a multiple of 8, >= the longest text + 8
    uint32_t *dist;
    uint8_t *strand;
};

// The group's lanes call this together.  Pattern: bases [ps, ps + m) of record prec, 1 <= m; text: [ts, ts + n) of trec, m <= n.
// carry: the group's scratch row when the pattern has more than g blocks (nullptr otherwise).
__device__ void ed_pair(const RunTable &t, uint32_t prec, uint32_t ps, uint32_t m, uint32_t trec, uint32_t ts, uint32_t n, uint32_t g, uint32_t b,
                        uint8_t *carry, uint32_t *dist_out, uint8_t *strand_out)
{
    const uint32_t nb = (m + 63) >> 6, n_stripes = (nb + g - 1) / g;
    const uint64_t pbase = t.rec_base[prec] + ps, tbase = t.rec_base[trec] + ts;
    uint32_t score_f = m, score_r = m;
    RunMemo pm, tm;   // one memo per side: the pattern's record and the text's are different records as a rule
    for (uint32_t s = 0; s < n_stripes; ++s) {
        const uint32_t B = s * g + b, sb = nb - s * g < g ? nb - s * g : g;
        const bool active = b < sb, last_block = B == nb - 1, first = s == 0;
        const bool leaves_carry = active && b == sb - 1 && !last_block;
        // the block's rows as bit planes: low and high bit of the code, validity
        uint64_t lo = 0, hi = 0, vm = 0;
        if (active) {
            const uint32_t pos = 64 * B, cnt = m - pos < 64 ? m - pos : 64, c0 = cnt < 32 ? cnt : 32, c1 = cnt - c0;
            const uint64_t x0 = load_codes(t.packed, pbase + pos, c0);
            vm = valid32(t, prec, ps + pos, c0, pm);
            lo = even_bits(x0);
            hi = even_bits(x0 >> 1);
            if (c1) {
                const uint64_t x1 = load_codes(t.packed, pbase + pos + 32, c1);
                vm |= (uint64_t)valid32(t, prec, ps + pos + 32, c1, pm) << 32;
                lo |= (uint64_t)even_bits(x1) << 32;
                hi |= (uint64_t)even_bits(x1 >> 1) << 32;
            }
        }
        const uint32_t out_bit = last_block ? (m - 1) & 63u : 63u;
        uint64_t Pf = ~0ull, Mf = 0, Pr = ~0ull, Mr = 0;
        uint64_t tf = 0, tr = 0, cbuf = 0;   // lane 0: 32 columns of the text on either strand, 8 columns of the carry row
        uint32_t vf = 0, vr = 0, rcnt = 0;
        uint32_t msg = 0;                    // column base and delta of both strands: cf [0,3) hf [3,5) cr [5,8) hr [8,10)
        const uint32_t steps = n + sb - 1;
        for (uint32_t step = 0; step < steps; ++step) {
            uint32_t in = __shfl_up(msg, 1, g);
            if (b == 0 && step < n) {
                const uint32_t i = step & 31u;
                if (i == 0) {
                    const uint32_t cnt = n - step < 32 ? n - step : 32;
                    tf = load_codes(t.packed, tbase + step, cnt);
                    vf = valid32(t, trec, ts + step, cnt, tm);
                    // the reverse complement's columns step .. step + cnt - 1 are positions top - 1 down to top - cnt
                    const uint32_t top = n - step;
                    rcnt = cnt;
                    tr = load_codes(t.packed, tbase + (top - cnt), cnt);
                    vr = valid32(t, trec, ts + (top - cnt), cnt, tm);
                }
                const uint32_t j = rcnt - 1 - i;
                const uint32_t cf = ((vf >> i) & 1u) ? (uint32_t)(tf >> (2 * i)) & 3u : 4u;
                const uint32_t cr = ((vr >> j) & 1u) ? 3u - ((uint32_t)(tr >> (2 * j)) & 3u) : 4u;
                uint32_t hf = 1, hr = 1;   // the top row of the table rises by one per column
                if (!first) {
                    if ((step & 7u) == 0) cbuf = *reinterpret_cast<const uint64_t *>(carry + step);
                    const uint32_t c = (uint32_t)(cbuf >> (8 * (step & 7u))) & 0xFFu;
                    hf = c & 3u;
                    hr = (c >> 2) & 3u;
                }
                in = cf | (hf << 3) | (cr << 5) | (hr << 8);
            }
            const uint32_t col = step - b;   // (wraps below zero: then >= n)
            if (active && step >= b && col < n) {
                const uint32_t cf = in & 7u, hf = (in >> 3) & 3u, cr = (in >> 5) & 7u, hr = (in >> 8) & 3u;
                const uint64_t ef = cf < 4 ? ~(lo ^ (0ull - (cf & 1u))) & ~(hi ^ (0ull - ((cf >> 1) & 1u))) & vm : 0ull;
                const uint64_t er = cr < 4 ? ~(lo ^ (0ull - (cr & 1u))) & ~(hi ^ (0ull - ((cr >> 1) & 1u))) & vm : 0ull;
                const uint32_t of = myers_step(ef, Pf, Mf, hf, out_bit), orr = myers_step(er, Pr, Mr, hr, out_bit);
                if (last_block) {
                    score_f += of == 1 ? 1u : of == 2 ? 0xFFFFFFFFu : 0u;
                    score_r += orr == 1 ? 1u : orr == 2 ? 0xFFFFFFFFu : 0u;
                } else if (leaves_carry) {
                    carry[col] = (uint8_t)(of | (orr << 2));   // (read by lane 0 of the next stripe, which is past this column there)
                }
                msg = cf | (of << 3) | (cr << 5) | (orr << 8);
            }
        }
        if (n_stripes > 1) __threadfence();   // the row is complete and visible before the next stripe reads it
        if (active && last_block) {
            *dist_out = score_f <= score_r ? score_f : score_r;
            *strand_out = score_f <= score_r ? 0 : 1;
        }
    }
}

// pattern = the shorter side (R on a tie)
__device__ __forceinline__ void ed_sides(const sw_interval &r, const sw_interval &s, uint32_t &prec, uint32_t &ps, uint32_t &m, uint32_t &trec,
                                         uint32_t &ts, uint32_t &n)
{
    const uint32_t lr = r.stop - r.start, ls = s.stop - s.start;
    const bool swap = ls < lr;
    prec = swap ? s.record : r.record;
    ps = swap ? s.start : r.start;
    m = swap ? ls : lr;
    trec = swap ? r.record : s.record;
    ts = swap ? r.start : s.start;
    n = swap ? lr : ls;
}

// register route: group x of the launch does pair list[x]
__global__ __launch_bounds__(SQ_TPB) void k_ed(EdArgs a)
{
    const uint64_t tid = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x, grp = tid / a.g;
    if (grp >= a.count) return;   // (whole groups)
    const uint32_t i = a.list[grp];
    uint32_t prec, ps, m, trec, ts, n;
    ed_sides(a.R[i], a.S[i], prec, ps, m, trec, ts, n);
    ed_pair(a.t, prec, ps, m, trec, ts, n, a.g, (uint32_t)(tid % a.g), nullptr, a.dist + i, a.strand + i);
}

// striped route: group x of the launch does pairs list[x], list[x + groups], ... with row x of the scratch
__global__ __launch_bounds__(SQ_TPB) void k_ed_striped(EdArgs a, uint32_t groups)
{
    const uint64_t tid = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x, grp = tid / a.g;
    if (grp >= groups) return;
    for (uint64_t x = grp; x < a.count; x += groups) {
        const uint32_t i = a.list[x];
        uint32_t prec, ps, m, trec, ts, n;
        ed_sides(a.R[i], a.S[i], prec, ps, m, trec, ts, n);
        ed_pair(a.t, prec, ps, m, trec, ts, n, a.g, (uint32_t)(tid % a.g), a.carry + grp * a.carry_stride, a.dist + i, a.strand + i);
        __threadfence();   // (the row is reused by the group's next pair)
    }
}

// A pair with an empty side is answered here; every other one is appended to the list of its class.
// stat[0 .. 7]: entries of the class lists, [8] sum of |R| |S|, [9] longest side, [10] longest text of the striped class
__global__ __launch_bounds__(SQ_TPB) void k_ed_classify(const sw_interval *__restrict__ R, const sw_interval *__restrict__ S, uint64_t n, uint32_t cap,
                                                        uint32_t *__restrict__ lists, unsigned long long *__restrict__ stat, uint32_t *__restrict__ dist,
                                                        uint8_t *__restrict__ strand)
{
    const uint64_t i = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x;
    const uint32_t lane = threadIdx.x % SQ_WAVE;
    uint32_t cls = ED_CLASSES, longer = 0;
    unsigned long long cells = 0;
    if (i < n) {
        const uint32_t lr = R[i].stop - R[i].start, ls = S[i].stop - S[i].start, m = lr < ls ? lr : ls;
        longer = lr < ls ? ls : lr;
        cells = (unsigned long long)lr * ls;
        if (m == 0) {
            dist[i] = longer;
            strand[i] = 0;
        } else {
            const uint32_t nb = (m + 63) >> 6;
            cls = 0;
            if (nb > cap) cls = ED_CLASSES - 1;
            else
                while ((1u << cls) < nb) ++cls;
        }
    }
    for (uint32_t c = 0; c < ED_CLASSES; ++c) {
        const unsigned long long mask = __ballot(cls == c);
        if (!mask) continue;   // (uniform)
        unsigned long long at = 0;
        if (lane == (uint32_t)__ffsll((long long)mask) - 1) at = atomicAdd(stat + c, (unsigned long long)__popcll(mask));
        at = __shfl(at, __ffsll((long long)mask) - 1, SQ_WAVE);
        if (cls == c) lists[(uint64_t)c * n + at + __popcll(mask & ((1ull << lane) - 1))] = (uint32_t)i;
    }
    for (uint32_t d = SQ_WAVE / 2; d; d >>= 1) cells += __shfl_down(cells, d, SQ_WAVE);
    if (lane == 0 && cells) atomicAdd(stat + 8, cells);
    if (longer) atomicMax(stat + 9, (unsigned long long)longer);
    if (cls == ED_CLASSES - 1) atomicMax(stat + 10, (unsigned long long)longer);
}

// ---- the interval lists of a sw_markers -----------------------------------------------------------------------------------------
__device__ __forceinline__ sw_interval iv_of(const sw_marker_row &r, const uint32_t *ro)
{
    return sw_interval{ro[r.assembly_idx] + r.record_idx, r.start, r.stop};
}

__global__ void k_mk_reps(const sw_marker_rep *reps, const uint64_t *sel, uint64_t n_sel, const uint32_t *ro, sw_interval *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_sel) out[i] = iv_of(reps[sel[i]].row, ro);
}

// row j of the output is row row_off[sel[k]] + (j - dst_off[k]) of the table, k the selected subgraph whose range holds j
__global__ void k_mk_rows(const sw_marker_rep *reps, const sw_marker_row *rows, const uint64_t *row_off, const uint64_t *sel, const uint64_t *dst_off,
                          uint64_t n_sel, uint64_t n_out, const uint32_t *ro, sw_interval *rep_out, sw_interval *row_out)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    uint64_t lo = 0, hi = n_sel;   // the last k with dst_off[k] <= j
    while (lo + 1 < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (dst_off[mid] <= j) lo = mid; else hi = mid;
    }
    const uint64_t s = sel[lo];
    row_out[j] = iv_of(rows[row_off[s] + (j - dst_off[lo])], ro);
    if (rep_out) rep_out[j] = iv_of(reps[s].row, ro);
}

}  // namespace
}  // namespace sw

struct sw_seqs {
    int device = 0;
    uint64_t n = 0, bytes = 0;
    sw::DevArray<uint64_t> off;     // [n + 1]
    sw::DevArray<char> blob;        // [bytes]
    sw::DevArray<uint8_t> flags;    // [n]
    uint64_t counters[2] = {};      // launches of the decode kernel, bytes written
    double ms[1] = {};              // checks, offsets and decode (HIP events)
};

namespace sw {
namespace {

// the text of n checked intervals (device list)
void fetch_device(const DevRuns &runs, const sw_interval *d_iv, uint64_t n, sw_seqs &o)
{
    Event e0, e1;
    SW_HIP(hipEventRecord(e0, SQ_STREAM));
    check_intervals(runs.t, d_iv, n, "fetch");
    o.n = n;
    o.off.alloc(n + 1);
    o.flags.alloc(n);
    {
        size_t tmp_bytes = 0;
        auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), IvLenAt{d_iv, n});
        SW_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, in, o.off.p, uint64_t(0), n + 1, rocprim::plus<uint64_t>(), SQ_STREAM));
        DevArray<unsigned char> tmp(tmp_bytes);
        SW_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, in, o.off.p, uint64_t(0), n + 1, rocprim::plus<uint64_t>(), SQ_STREAM));
        SW_HIP(hipMemcpy(&o.bytes, o.off.p + n, 8, hipMemcpyDeviceToHost));
    }
    o.blob.alloc(o.bytes);
    // a launch holds at most launch_blocks(SQ_BLOCKS_ENV) workgroups (fewer than 2^32 threads) and SQ_PER_WAVE intervals per wave
    const uint64_t per_launch = (uint64_t)launch_blocks(SQ_BLOCKS_ENV) * SQ_WPB * SQ_PER_WAVE;
    uint64_t launches = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += per_launch, ++launches) {
        const uint64_t i1 = std::min<uint64_t>(n, i0 + per_launch);
        const uint64_t blocks = std::min<uint64_t>(launch_blocks(SQ_BLOCKS_ENV), (i1 - i0 + SQ_WPB - 1) / SQ_WPB);
        hipLaunchKernelGGL(k_fetch, dim3((unsigned)blocks), dim3(SQ_TPB), 0, SQ_STREAM, runs.t, d_iv, o.off.p, i0, i1, o.blob.p, o.flags.p);
        SW_HIP(hipGetLastError());
    }
    SW_HIP(hipEventRecord(e1, SQ_STREAM));
    SW_HIP(hipStreamSynchronize(SQ_STREAM));
    float ms = 0;
    SW_HIP(hipEventElapsedTime(&ms, e0, e1));
    o.ms[0] = ms;
    o.counters[0] = launches;
    o.counters[1] = o.bytes;
}

// dist / strand of n checked pairs (device lists, device outputs)
void distances_device(const DevRuns &runs, const sw_interval *d_R, const sw_interval *d_S, uint64_t n, uint32_t *d_dist, uint8_t *d_strand,
                      uint64_t *counters, double *ms_out)
{
    Event e0, e1, e2;
    SW_HIP(hipEventRecord(e0, SQ_STREAM));
    check_intervals(runs.t, d_R, n, "edit distances (R)");
    check_intervals(runs.t, d_S, n, "edit distances (S)");
    const uint32_t cap = ed_cap_blocks();
    unsigned long long stat[11] = {};
    uint64_t launches = 0;
    if (n) {
        DevArray<uint32_t> lists((uint64_t)ED_CLASSES * n);
        DevArray<unsigned long long> d_stat(11);
        SW_HIP(hipMemsetAsync(d_stat.p, 0, sizeof stat, SQ_STREAM));
        hipLaunchKernelGGL(k_ed_classify, dim3(sq_blocks(n)), dim3(SQ_TPB), 0, SQ_STREAM, d_R, d_S, n, cap, lists.p, d_stat.p, d_dist, d_strand);
        SW_HIP(hipGetLastError());
        SW_HIP(hipMemcpyAsync(stat, d_stat.p, sizeof stat, hipMemcpyDeviceToHost, SQ_STREAM));
        SW_HIP(hipEventRecord(e1, SQ_STREAM));
        SW_HIP(hipStreamSynchronize(SQ_STREAM));
        EdArgs a{};
        a.t = runs.t;
        a.R = d_R;
        a.S = d_S;
        a.dist = d_dist;
        a.strand = d_strand;
        const uint64_t max_threads = (uint64_t)launch_blocks(SQ_BLOCKS_ENV) * SQ_TPB;
        for (uint32_t c = 0; c + 1 < ED_CLASSES; ++c) {   // register route, g = 2^c lanes per pair
            const uint64_t cnt = stat[c], g = 1ull << c, per_launch = std::max<uint64_t>(max_threads / g, 1);
            for (uint64_t x0 = 0; x0 < cnt; x0 += per_launch, ++launches) {
                a.list = lists.p + (uint64_t)c * n + x0;
                a.count = std::min<uint64_t>(per_launch, cnt - x0);
                a.g = (uint32_t)g;
                hipLaunchKernelGGL(k_ed, dim3(sq_blocks(a.count * g)), dim3(SQ_TPB), 0, SQ_STREAM, a);
                SW_HIP(hipGetLastError());
            }
        }
        DevArray<uint8_t> scratch;
        if (const uint64_t cnt = stat[ED_CLASSES - 1]) {   // striped route: the largest power of two <= cap lanes per pair
            uint32_t g = 1;
            while (g * 2 <= cap) g *= 2;
            const uint32_t groups = (uint32_t)std::min<uint64_t>({cnt, (uint64_t)ED_STRIPE_GROUPS, std::max<uint64_t>(max_threads / g, 1)});
            a.carry_stride = ((uint64_t)stat[10] + 15) & ~7ull;
            scratch.alloc((uint64_t)groups * a.carry_stride);
            a.carry = scratch.p;
            a.list = lists.p + (uint64_t)(ED_CLASSES - 1) * n;
            a.count = cnt;
            a.g = g;
            hipLaunchKernelGGL(k_ed_striped, dim3(sq_blocks((uint64_t)groups * g)), dim3(SQ_TPB), 0, SQ_STREAM, a, groups);
            SW_HIP(hipGetLastError());
            ++launches;
        }
        SW_HIP(hipEventRecord(e2, SQ_STREAM));
        SW_HIP(hipStreamSynchronize(SQ_STREAM));   // (lists / scratch go back to the pool behind the kernels)
    } else {
        SW_HIP(hipEventRecord(e1, SQ_STREAM));
        SW_HIP(hipEventRecord(e2, SQ_STREAM));
        SW_HIP(hipStreamSynchronize(SQ_STREAM));
    }
    if (counters) {
        const uint64_t cn[6] = {n, stat[8], stat[ED_CLASSES - 1], stat[9], launches, cap};
        memcpy(counters, cn, sizeof cn);
    }
    if (ms_out) {
        float ms = 0;
        SW_HIP(hipEventElapsedTime(&ms, e0, e1));
        ms_out[0] = ms;
        SW_HIP(hipEventElapsedTime(&ms, e1, e2));
        ms_out[1] = ms;
    }
}

// the batch's record table must start with the one the markers were located with: global record = record_offsets[assembly] + record_idx
void check_cover(const sw_markers &m, const sw_batch &b)
{
    const std::vector<uint32_t> &mo = m.record_offsets, &bo = b.host.record_offsets;
    if (mo.empty()) raise(SW_ERR_VALUE, "the markers carry no record table");
    if (bo.size() < mo.size())
        raise(SW_ERR_VALUE, "the batch's record table does not cover the markers' records: %llu assemblies in the batch, %llu behind the markers",
              (unsigned long long)(bo.empty() ? 0 : bo.size() - 1), (unsigned long long)(mo.size() - 1));
    for (size_t a = 0; a < mo.size(); ++a)
        if (mo[a] != bo[a])
            raise(SW_ERR_VALUE, "the batch's record table does not cover the markers' records: record_offsets[%llu] is %u in the batch, %u behind the markers",
                  (unsigned long long)a, bo[a], mo[a]);
    if (m.device != b.device) raise(SW_ERR_VALUE, "the markers and the batch live on different devices (%d, %d)", m.device, b.device);
}

struct MarkerLists {
    DevArray<uint32_t> ro;
    DevArray<uint64_t> sel, dst_off;
    DevArray<sw_interval> reps, rows;
    uint64_t n = 0;
};

// rows == 0: the representatives of the selected subgraphs; rows != 0: their rows (pairs: with the representative beside each row)
void marker_lists(const sw_markers &m, const sw_batch &b, int rows, bool pairs, const uint64_t *sel, uint64_t n_sel, MarkerLists &L)
{
    check_cover(m, b);
    if (n_sel && !sel) raise(SW_ERR_VALUE, "a NULL array");
    if (n_sel > SQ_MAX_LIST) raise(SW_ERR_VALUE, "%llu selected subgraphs exceed one launch of the list kernels (%llu)", (unsigned long long)n_sel, (unsigned long long)SQ_MAX_LIST);
    for (uint64_t i = 0; i < n_sel; ++i)
        if (sel[i] >= m.n_sg) raise(SW_ERR_VALUE, "select[%llu] = %llu is no subgraph (%llu)", (unsigned long long)i, (unsigned long long)sel[i], (unsigned long long)m.n_sg);
    if (rows && !m.keep_rows) raise(SW_ERR_VALUE, "the rows were not kept (keep_rows = 0)");
    const std::vector<uint32_t> &bo = b.host.record_offsets;
    L.ro.alloc(bo.size());
    SW_HIP(hipMemcpyAsync(L.ro.p, bo.data(), bo.size() * 4, hipMemcpyHostToDevice, SQ_STREAM));
    L.sel.alloc(n_sel);
    if (n_sel) SW_HIP(hipMemcpyAsync(L.sel.p, sel, n_sel * 8, hipMemcpyHostToDevice, SQ_STREAM));
    if (!rows) {
        L.n = n_sel;
        L.reps.alloc(n_sel);
        if (n_sel) hipLaunchKernelGGL(k_mk_reps, dim3(sq_blocks(n_sel)), dim3(SQ_TPB), 0, SQ_STREAM, m.reps.p, L.sel.p, n_sel, L.ro.p, L.reps.p);
        SW_HIP(hipGetLastError());
        SW_HIP(hipStreamSynchronize(SQ_STREAM));
        return;
    }
    std::vector<uint64_t> row_off(m.n_sg + 1), dst(n_sel + 1, 0);
    SW_HIP(hipMemcpy(row_off.data(), m.row_off.p, (m.n_sg + 1) * 8, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n_sel; ++i) dst[i + 1] = dst[i] + (row_off[sel[i] + 1] - row_off[sel[i]]);
    L.n = dst[n_sel];
    if (L.n > SQ_MAX_LIST) raise(SW_ERR_VALUE, "%llu rows exceed one launch of the list kernels (%llu)", (unsigned long long)L.n, (unsigned long long)SQ_MAX_LIST);
    L.dst_off.alloc(n_sel + 1);
    SW_HIP(hipMemcpyAsync(L.dst_off.p, dst.data(), (n_sel + 1) * 8, hipMemcpyHostToDevice, SQ_STREAM));
    L.rows.alloc(L.n);
    if (pairs) L.reps.alloc(L.n);
    if (L.n)
        hipLaunchKernelGGL(k_mk_rows, dim3(sq_blocks(L.n)), dim3(SQ_TPB), 0, SQ_STREAM, m.reps.p, m.rows.p, m.row_off.p, L.sel.p, L.dst_off.p, n_sel, L.n,
                           L.ro.p, pairs ? L.reps.p : (sw_interval *)nullptr, L.rows.p);
    SW_HIP(hipGetLastError());
    SW_HIP(hipStreamSynchronize(SQ_STREAM));   // (dst is a local)
}

void download_distances(const DevArray<uint32_t> &d_dist, const DevArray<uint8_t> &d_strand, uint64_t n, uint32_t *dist, uint8_t *strand)
{
    if (!n) return;
    if (dist) SW_HIP(hipMemcpy(dist, d_dist.p, n * 4, hipMemcpyDeviceToHost));
    if (strand) SW_HIP(hipMemcpy(strand, d_strand.p, n, hipMemcpyDeviceToHost));
}

}  // namespace
}  // namespace sw

using namespace sw;

extern "C" {

int sw_batch_fetch(const sw_batch *b, const sw_interval *intervals, uint64_t n, sw_seqs **out)
{
    return guarded([&] {
        if (!b || !out || (n && !intervals)) raise(SW_ERR_VALUE, "fetch: a NULL handle or array");
        require_device(b->device, "the batch");
        StreamScope scope(SQ_STREAM);
        DevRuns runs(*b);
        DevArray<sw_interval> d_iv(n);
        if (n) SW_HIP(hipMemcpyAsync(d_iv.p, intervals, n * sizeof(sw_interval), hipMemcpyHostToDevice, SQ_STREAM));
        std::unique_ptr<sw_seqs> o(new sw_seqs);
        o->device = b->device;
        fetch_device(runs, d_iv.p, n, *o);
        *out = o.release();
    });
}

int sw_markers_fetch(const sw_markers *m, const sw_batch *b, int rows, const uint64_t *select, uint64_t n_select, sw_seqs **out)
{
    return guarded([&] {
        if (!m || !b || !out) raise(SW_ERR_VALUE, "fetch: a NULL handle");
        require_device(b->device, "the batch");
        StreamScope scope(SQ_STREAM);
        MarkerLists L;
        marker_lists(*m, *b, rows, false, select, n_select, L);
        DevRuns runs(*b);
        std::unique_ptr<sw_seqs> o(new sw_seqs);
        o->device = b->device;
        fetch_device(runs, rows ? L.rows.p : L.reps.p, L.n, *o);
        *out = o.release();
    });
}

int sw_seqs_sizes(const sw_seqs *s, uint64_t *n, uint64_t *bytes)
{
    return guarded([&] {
        if (!s) raise(SW_ERR_VALUE, "fetch: a NULL handle");
        if (n) *n = s->n;
        if (bytes) *bytes = s->bytes;
    });
}

int sw_seqs_export(const sw_seqs *s, uint64_t *offsets, char *blob, uint8_t *flags)
{
    return guarded([&] {
        if (!s) raise(SW_ERR_VALUE, "fetch: a NULL handle");
        require_device(s->device, "the sequences");
        if (offsets) SW_HIP(hipMemcpy(offsets, s->off.p, (s->n + 1) * 8, hipMemcpyDeviceToHost));
        if (blob && s->bytes) SW_HIP(hipMemcpy(blob, s->blob.p, s->bytes, hipMemcpyDeviceToHost));
        if (flags && s->n) SW_HIP(hipMemcpy(flags, s->flags.p, s->n, hipMemcpyDeviceToHost));
    });
}

int sw_seqs_stats(const sw_seqs *s, uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (!s) raise(SW_ERR_VALUE, "fetch: a NULL handle");
        if (counters) memcpy(counters, s->counters, sizeof s->counters);
        if (ms) memcpy(ms, s->ms, sizeof s->ms);
    });
}

void sw_seqs_free(sw_seqs *s)
{
    delete s;
}

int sw_batch_edit_distances(const sw_batch *b, const sw_interval *r, const sw_interval *s, uint64_t n, uint32_t *dist, uint8_t *strand,
                            uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (!b || (n && (!r || !s || !dist || !strand))) raise(SW_ERR_VALUE, "edit distances: a NULL handle or array");
        require_device(b->device, "the batch");
        StreamScope scope(SQ_STREAM);
        DevRuns runs(*b);
        DevArray<sw_interval> d_R(n), d_S(n);
        DevArray<uint32_t> d_dist(n);
        DevArray<uint8_t> d_strand(n);
        if (n) {
            SW_HIP(hipMemcpyAsync(d_R.p, r, n * sizeof(sw_interval), hipMemcpyHostToDevice, SQ_STREAM));
            SW_HIP(hipMemcpyAsync(d_S.p, s, n * sizeof(sw_interval), hipMemcpyHostToDevice, SQ_STREAM));
        }
        distances_device(runs, d_R.p, d_S.p, n, d_dist.p, d_strand.p, counters, ms);
        download_distances(d_dist, d_strand, n, dist, strand);
    });
}

int sw_markers_row_distances(const sw_markers *m, const sw_batch *b, const uint64_t *select, uint64_t n_select, uint32_t *dist, uint8_t *strand,
                             uint64_t *counters, double *ms)
{
    return guarded([&] {
        if (!m || !b) raise(SW_ERR_VALUE, "edit distances: a NULL handle");
        require_device(b->device, "the batch");
        StreamScope scope(SQ_STREAM);
        MarkerLists L;
        marker_lists(*m, *b, 1, true, select, n_select, L);
        if (L.n && (!dist || !strand)) raise(SW_ERR_VALUE, "edit distances: a NULL array");
        DevRuns runs(*b);
        DevArray<uint32_t> d_dist(L.n);
        DevArray<uint8_t> d_strand(L.n);
        distances_device(runs, L.reps.p, L.rows.p, L.n, d_dist.p, d_strand.p, counters, ms);
        download_distances(d_dist, d_strand, L.n, dist, strand);
    });
}

}  // extern "C"
