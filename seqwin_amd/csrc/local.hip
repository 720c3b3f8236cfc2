// local.hip -- the optimal LOCAL alignment of a query against an interval of the batch under a reward / penalty / gap-open /
// gap-extend scoring system (Smith-Waterman with Gotoh's affine gaps), for every pair on which Layer A (hits.hip) runs.
//
// No counterpart in the reference: NOT BLAST.  The seeds and the window are ours, the dynamic programme is exhaustive inside the
// window (no X-drop), there is no e-value filter and none of MarkerMetrics is filled.  DESIGN.md section 3.2i is the specification;
// tests/tools/local_host.py restates it twice.
//
// There is no stored matrix and no traceback: every H, E and F value carries a record (i0, j0, mismatch, gapopen, gaps) forward.
//   k_lc_classify  pairs with an empty side answered; the others listed by the power of two >= the query's strips of LC_R rows,
//                  or by the striped route (carry row in LDS where the text fits the bound, in HBM above it)
//   k_lc           an integer systolic wavefront: a group of 2^c lanes works on one pair, lane l owns LC_R consecutive pattern rows
//                  (H, E and their records in registers, the rows unrolled) and is at text column t - l in step t; the strip's
//                  bottom H, F and records go to lane l + 1 by __shfl_up.  Every lane keeps its running maximum; the group reduces
//                  them by (score descending, j ascending, i ascending)
//   k_lc_striped   queries above one group pass (lanes x LC_R rows): passes one below the other, a carry row of (H, F, records)
//                  per text column between them; a workgroup is one group
#include "hits_core.hpp"

namespace sw {
namespace {

constexpr uint32_t LC_R = 8;                        // pattern rows per lane: speed only, no measurement behind it
constexpr uint32_t LC_MAX_LANES = 64;               // lanes of the widest group: a wave
constexpr uint32_t LC_CLASSES = 9;                  // group widths 1, 2, ... 64, then striped with an LDS row, striped with an HBM row
constexpr uint32_t LC_CLS_LDS = 7, LC_CLS_HBM = 8;
constexpr uint32_t LC_STRIPE_GROUPS = 1024;         // groups of a launch of the striped route
constexpr uint64_t LC_LDS_BYTES = 32u << 10;        // the carry row's LDS bound per group: speed only, no measurement behind it
constexpr uint64_t LC_HBM_BYTES = 256ull << 20;     // the carry rows of one launch in HBM at most (one row is always granted)
constexpr uint32_t LC_CARRY_BYTES = 32;             // H, F and two records per text column
constexpr int32_t LC_NEG = -(1 << 30);              // minus infinity: below every value a finite chain of gaps reaches
constexpr uint32_t LC_FIELDS = 9;

// The record of a value.  org = i0 | j0 << 16 (both < 2^16); cnt = mismatch | gapopen << 16 | gaps << 33: mismatch < 2^16, gapopen and
// gaps < 2^17 (at most one gap column per row and per column), so the three counts never carry into each other.
struct Rec {
    uint32_t org;
    uint64_t cnt;
};
constexpr uint64_t LC_MM = 1ull, LC_OPEN = (1ull << 16) | (1ull << 33), LC_EXT = 1ull << 33;

// what a strip hands down per column: H and F of its bottom row with their records, and the column's base
struct Edge {
    uint32_t hc;   // H | base << 24 (H <= 255 * 65535 < 2^24)
    int32_t f;
    Rec rh, rf;
};

struct LcArgs {
    RunTable t;
    const uint32_t *codes[2], *valid[2];
    const uint64_t *qoff;
    const sw_infix_pair *pairs;
    const uint32_t *out_idx;   // where pair i's results go (nullptr: i)
    const uint32_t *list;      // pair indices of this launch's class
    uint64_t count;
    uint32_t g;                // lanes per pair (a power of two <= 64)
    uint4 *carry;              // HBM route: one row of carry_stride columns per group of the launch
    uint64_t carry_stride;
    int32_t r, p, go, ge;
    uint32_t *out[LC_FIELDS];  // score, qstart, qend, sstart, send, nident, mismatch, gapopen, gaps
};

__device__ __forceinline__ Edge shfl_up_edge(const Edge &e, uint32_t g)
{
    Edge o;
    o.hc = __shfl_up(e.hc, 1, g);
    o.f = __shfl_up(e.f, 1, g);
    o.rh.org = __shfl_up(e.rh.org, 1, g);
    o.rh.cnt = __shfl_up((unsigned long long)e.rh.cnt, 1, g);
    o.rf.org = __shfl_up(e.rf.org, 1, g);
    o.rf.cnt = __shfl_up((unsigned long long)e.rf.cnt, 1, g);
    return o;
}

// a lane's running maximum: the first cell in (j, i) order that attains it
struct Best {
    int32_t score = 0;
    uint32_t i = 0, j = 0;
    Rec rec{0, 0};
};

__device__ __forceinline__ bool better(int32_t s, uint32_t j, uint32_t i, const Best &b)
{
    return s > b.score || (s == b.score && (j < b.j || (j == b.j && i < b.i)));
}

// The group's lanes call this together.  Pattern: strand p.strand of query p.query, m >= 1 bases; text: [p.start, p.stop), n >= 1.
// carry: the group's row of n columns (nullptr on the register route, where one pass holds the query).
__device__ __forceinline__ void local_pair(const LcArgs &a, uint32_t pi, uint32_t g, uint32_t l, uint4 *carry)
{
    const RunTable &t = a.t;
    const sw_infix_pair p = a.pairs[pi];
    const uint64_t qbase = a.qoff[p.query];
    const uint32_t m = (uint32_t)(a.qoff[p.query + 1] - qbase), n = p.stop - p.start;
    const uint32_t *codes = a.codes[p.strand & 1u], *valid = a.valid[p.strand & 1u];
    const uint32_t pass = g * LC_R, n_stripes = (m + pass - 1) / pass;
    const uint64_t tbase = t.rec_base[p.record] + p.start;
    const int32_t r = a.r, pen = a.p, go = a.go, ge = a.ge;
    Best best;
    RunMemo tm;
    for (uint32_t s = 0; s < n_stripes; ++s) {
        const uint32_t base = s * pass, left = m - base, sl = left >= pass ? g : (left + LC_R - 1) / LC_R;   // lanes with rows
        const uint32_t row0 = base + l * LC_R, nr = row0 >= m ? 0u : (m - row0 < LC_R ? m - row0 : LC_R);
        const bool first = s == 0, leaves_carry = s + 1 < n_stripes && l == g - 1;
        // the strip's rows: 4 bits each, the base's code or 7 for an invalid base and for a row behind the query
        uint32_t prow = 0x77777777u;
        if (nr) {
            const uint64_t x = load_codes(codes, qbase + row0, nr);
            const uint32_t v = plane32(valid, qbase + row0, nr);
#pragma unroll
            for (uint32_t k = 0; k < LC_R; ++k)
                if ((v >> k) & 1u) prow = (prow & ~(0xFu << (4 * k))) | (((uint32_t)(x >> (2 * k)) & 3u) << (4 * k));
        }
        int32_t H[LC_R], E[LC_R];
        Rec rH[LC_R], rE[LC_R];
#pragma unroll
        for (uint32_t k = 0; k < LC_R; ++k) {   // column 0
            H[k] = 0;
            rH[k] = Rec{row0 + k + 1, 0};
            E[k] = LC_NEG;
            rE[k] = Rec{0, 0};
        }
        int32_t dH = 0;            // H of the row above the strip in the previous column, and its record
        Rec dR{row0, 0};
        Edge msg{0, 0, Rec{0, 0}, Rec{0, 0}};
        uint64_t tf = 0;           // lane 0: 32 columns of the text
        uint32_t vf = 0;
        const uint32_t steps = n + sl - 1;
        for (uint32_t step = 0; step < steps; ++step) {
            Edge in = shfl_up_edge(msg, g);
            if (l == 0 && step < n) {
                const uint32_t x = step & 31u;
                if (x == 0) {
                    const uint32_t cnt = n - step < 32 ? n - step : 32;
                    tf = load_codes(t.packed, tbase + step, cnt);
                    vf = valid32(t, p.record, p.start + step, cnt, tm);
                }
                const uint32_t cf = ((vf >> x) & 1u) ? (uint32_t)(tf >> (2 * x)) & 3u : 4u;
                if (first) {   // row 0 of the table: H = 0 everywhere, F = minus infinity
                    in.hc = 0;
                    in.f = LC_NEG;
                    in.rh = Rec{(step + 1) << 16, 0};
                    in.rf = Rec{0, 0};
                } else {
                    const uint4 c0 = carry[2 * (uint64_t)step], c1 = carry[2 * (uint64_t)step + 1];
                    in.hc = c0.x;
                    in.f = (int32_t)c0.y;
                    in.rh = Rec{c0.z, (uint64_t)c1.x | (uint64_t)c1.y << 32};
                    in.rf = Rec{c0.w, (uint64_t)c1.z | (uint64_t)c1.w << 32};
                }
                in.hc = (in.hc & 0xFFFFFFu) | (cf << 24);
            }
            const uint32_t col = step - l + 1;   // 1-based (wraps below zero: then > n)
            if (nr && step >= l && col <= n) {
                const uint32_t cf = in.hc >> 24;
                int32_t uH = (int32_t)(in.hc & 0xFFFFFFu), uF = in.f;   // the cell above in this column
                Rec uRh = in.rh, uRf = in.rf;
                const int32_t top_h = uH;
                const Rec top_r = uRh;
#pragma unroll
                for (uint32_t k = 0; k < LC_R; ++k) {
                    const uint32_t i = row0 + k + 1;
                    const int32_t eo = H[k] - go, fo = uH - go;
                    const bool e_ext = E[k] >= eo, f_ext = uF >= fo;   // extension wins a tie
                    const int32_t e = (e_ext ? E[k] : eo) - ge, f = (f_ext ? uF : fo) - ge;
                    const Rec re{e_ext ? rE[k].org : rH[k].org, e_ext ? rE[k].cnt + LC_EXT : rH[k].cnt + LC_OPEN};
                    const Rec rf{f_ext ? uRf.org : uRh.org, f_ext ? uRf.cnt + LC_EXT : uRh.cnt + LC_OPEN};
                    const bool match = ((prow >> (4 * k)) & 7u) == cf;
                    int32_t h = dH + (match ? r : pen);
                    Rec rh{dR.org, dR.cnt + (match ? 0ull : LC_MM)};
                    if (e > h) {   // the first candidate that attains the maximum: diagonal, E, F
                        h = e;
                        rh = re;
                    }
                    if (f > h) {
                        h = f;
                        rh = rf;
                    }
                    if (h <= 0) {
                        h = 0;
                        rh = Rec{i | col << 16, 0};
                    }
                    dH = H[k];
                    dR = rH[k];
                    H[k] = h;
                    rH[k] = rh;
                    E[k] = e;
                    rE[k] = re;
                    uH = h;
                    uF = f;
                    uRh = rh;
                    uRf = rf;
                    if (k < nr && better(h, col, i, best)) {
                        best.score = h;
                        best.i = i;
                        best.j = col;
                        best.rec = rh;
                    }
                }
                dH = top_h;   // the next column's diagonal of the strip's first row
                dR = top_r;
                msg.hc = (uint32_t)uH | (cf << 24);
                msg.f = uF;
                msg.rh = uRh;
                msg.rf = uRf;
                if (leaves_carry) {   // (read by lane 0 of the next stripe, which is past this column there)
                    carry[2 * (uint64_t)(col - 1)] = make_uint4((uint32_t)uH, (uint32_t)uF, uRh.org, uRf.org);
                    carry[2 * (uint64_t)(col - 1) + 1] = make_uint4((uint32_t)uRh.cnt, (uint32_t)(uRh.cnt >> 32), (uint32_t)uRf.cnt, (uint32_t)(uRf.cnt >> 32));
                }
            }
        }
        if (n_stripes > 1) __threadfence();   // the row is complete and visible before the next stripe reads it
    }
    // the group's maximum: (score descending, j ascending, i ascending)
    for (uint32_t d = g >> 1; d; d >>= 1) {
        Best o;
        o.score = __shfl_xor(best.score, d, g);
        o.i = __shfl_xor(best.i, d, g);
        o.j = __shfl_xor(best.j, d, g);
        o.rec.org = __shfl_xor(best.rec.org, d, g);
        o.rec.cnt = __shfl_xor((unsigned long long)best.rec.cnt, d, g);
        if (better(o.score, o.j, o.i, best)) best = o;
    }
    if (l == 0) {
        const uint32_t oi = a.out_idx ? a.out_idx[pi] : pi;
        uint32_t v[LC_FIELDS] = {0, 0, 0, p.start, p.start, 0, 0, 0, 0};
        if (best.score > 0) {
            const uint32_t i0 = best.rec.org & 0xFFFFu, j0 = best.rec.org >> 16;
            const uint32_t mm = (uint32_t)(best.rec.cnt & 0xFFFFu), op = (uint32_t)(best.rec.cnt >> 16) & 0x1FFFFu, gp = (uint32_t)(best.rec.cnt >> 33);
            const uint32_t rows = best.i - i0, cols = best.j - j0, ins = (gp + rows - cols) >> 1;
            v[0] = (uint32_t)best.score;
            v[1] = i0;
            v[2] = best.i;
            v[3] = p.start + j0;
            v[4] = p.start + best.j;
            v[5] = rows - mm - ins;
            v[6] = mm;
            v[7] = op;
            v[8] = gp;
        }
#pragma unroll
        for (uint32_t f = 0; f < LC_FIELDS; ++f) a.out[f][oi] = v[f];
    }
}

// register route: group x of the launch does pair list[x]
__global__ __launch_bounds__(SQ_TPB) void k_lc(LcArgs a)
{
    const uint64_t tid = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x, grp = tid / a.g;
    if (grp >= a.count) return;   // (whole groups)
    local_pair(a, a.list[grp], a.g, (uint32_t)(tid % a.g), nullptr);
}

// striped route: a workgroup is one group of a.g lanes; group x does pairs list[x], list[x + groups], ... with its own carry row
template <bool LDS> __global__ __launch_bounds__(LC_MAX_LANES) void k_lc_striped(LcArgs a)
{
    extern __shared__ uint4 lc_row[];
    uint4 *carry = LDS ? lc_row : a.carry + 2 * (uint64_t)blockIdx.x * a.carry_stride;
    for (uint64_t x = blockIdx.x; x < a.count; x += gridDim.x) {
        local_pair(a, a.list[x], a.g, threadIdx.x, carry);
        __threadfence();   // (the row is reused by the group's next pair)
    }
}

// A pair with an empty side is answered here (score 0); every other one is appended to the list of its class.
// stat[0 .. 8]: entries of the class lists, [9] sum of |query| |text|, [10] / [11] longest text of the LDS / HBM class
__global__ __launch_bounds__(SQ_TPB) void k_lc_classify(const sw_infix_pair *__restrict__ pairs, const uint32_t *__restrict__ out_idx, const uint64_t *__restrict__ qoff,
                                                        uint64_t n, uint32_t max_lanes, uint32_t lds_cols, uint32_t *__restrict__ lists,
                                                        unsigned long long *__restrict__ stat, LcArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * SQ_TPB + threadIdx.x;
    const uint32_t lane = threadIdx.x % SQ_WAVE;
    uint32_t cls = LC_CLASSES, tn = 0;
    unsigned long long cells = 0;
    if (i < n) {
        const sw_infix_pair p = pairs[i];
        const uint32_t m = (uint32_t)(qoff[p.query + 1] - qoff[p.query]);
        tn = p.stop - p.start;
        cells = (unsigned long long)m * tn;
        if (m == 0 || tn == 0) {
            const uint32_t oi = out_idx ? out_idx[i] : (uint32_t)i;
#pragma unroll
            for (uint32_t f = 0; f < LC_FIELDS; ++f) a.out[f][oi] = (f == 3 || f == 4) ? p.start : 0u;
        } else {
            const uint32_t nl = (m + LC_R - 1) / LC_R;
            cls = 0;
            if (nl > max_lanes) cls = tn <= lds_cols ? LC_CLS_LDS : LC_CLS_HBM;
            else
                while ((1u << cls) < nl) ++cls;
        }
    }
    for (uint32_t c = 0; c < LC_CLASSES; ++c) {
        const unsigned long long mask = __ballot(cls == c);
        if (!mask) continue;   // (uniform)
        unsigned long long at = 0;
        if (lane == (uint32_t)__ffsll((long long)mask) - 1) at = atomicAdd(stat + c, (unsigned long long)__popcll(mask));
        at = __shfl(at, __ffsll((long long)mask) - 1, SQ_WAVE);
        if (cls == c) lists[(uint64_t)c * n + at + __popcll(mask & ((1ull << lane) - 1))] = (uint32_t)i;
    }
    for (uint32_t d = SQ_WAVE / 2; d; d >>= 1) cells += __shfl_down(cells, d, SQ_WAVE);
    if (lane == 0 && cells) atomicAdd(stat + 9, cells);
    const uint32_t longest_lds = wave_max(cls == LC_CLS_LDS ? tn : 0u), longest_hbm = wave_max(cls == LC_CLS_HBM ? tn : 0u);
    if (lane == 0 && longest_lds) atomicMax(stat + 10, (unsigned long long)longest_lds);
    if (lane == 0 && longest_hbm) atomicMax(stat + 11, (unsigned long long)longest_hbm);
}

}  // namespace

void check_scoring(const char *what, const sw_scoring *sc)
{
    if (!sc) raise(SW_ERR_VALUE, "%s: a NULL handle or array", what);
    if (sc->reward < 1 || sc->reward > 255 || sc->penalty < -255 || sc->penalty > -1 || sc->gapopen < 0 || sc->gapopen > 255 || sc->gapextend < 1 ||
        sc->gapextend > 255)
        raise(SW_ERR_VALUE, "%s: the scoring system (reward %d, penalty %d, gapopen %d, gapextend %d) lies outside 1..255, -255..-1, 0..255, 1..255", what,
              sc->reward, sc->penalty, sc->gapopen, sc->gapextend);
}

// the nine figures of n valid pairs (device list), every side below 2^16.  st is added to.
void local_device(const Runs &runs, const QueryPack &P, const sw_infix_pair *d_pairs, const uint32_t *d_out_idx, uint64_t n, const sw_scoring &sc,
                  uint32_t *const out[LOCAL_FIELDS], LocalStats &st)
{
    static_assert(LOCAL_FIELDS == LC_FIELDS, "the nine figures");
    const hipStream_t stream = HIT_STREAM;
    // rows of one group pass and the carry row's LDS bound change speed only; the test library lowers them
    uint64_t pass_rows = (uint64_t)LC_MAX_LANES * LC_R, lds_bytes = LC_LDS_BYTES;
    if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_LOCAL_ROWS")) pass_rows = std::min<uint64_t>(std::max<uint64_t>(env_u64(e, pass_rows), LC_R), pass_rows);
    if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_LOCAL_LDS_KB")) lds_bytes = std::min<uint64_t>(env_u64(e, lds_bytes >> 10) << 10, lds_bytes);
    uint32_t max_lanes = 1;   // the largest power of two of strips that fits the pass
    while (max_lanes * 2 * LC_R <= pass_rows) max_lanes *= 2;
    const uint32_t lds_cols = (uint32_t)(lds_bytes / LC_CARRY_BYTES);
    st.counters[5] = (uint64_t)max_lanes * LC_R;
    if (!n) return;
    if (n > SQ_MAX_LIST) raise(SW_ERR_VALUE, "local alignments: %llu pairs exceed one launch of the list kernels (%llu)", (unsigned long long)n, (unsigned long long)SQ_MAX_LIST);
    Event e0, e1;
    SW_HIP(hipEventRecord(e0, stream));
    LcArgs a{};
    a.t = table_of(runs);
    for (int s = 0; s < 2; ++s) {
        a.codes[s] = P.codes[s].p;
        a.valid[s] = P.valid[s].p;
    }
    a.qoff = P.off.p;
    a.pairs = d_pairs;
    a.out_idx = d_out_idx;
    a.r = sc.reward;
    a.p = sc.penalty;
    a.go = sc.gapopen;
    a.ge = sc.gapextend;
    for (uint32_t f = 0; f < LC_FIELDS; ++f) a.out[f] = out[f];
    unsigned long long stat[12] = {};
    DevArray<uint32_t> lists((uint64_t)LC_CLASSES * n);
    DevArray<unsigned long long> d_stat(12);
    SW_HIP(hipMemsetAsync(d_stat.p, 0, sizeof stat, stream));
    hipLaunchKernelGGL(k_lc_classify, dim3(sq_blocks(n)), dim3(SQ_TPB), 0, stream, d_pairs, d_out_idx, (const uint64_t *)P.off.p, n, max_lanes, lds_cols, lists.p,
                       d_stat.p, a);
    SW_HIP(hipGetLastError());
    SW_HIP(hipMemcpyAsync(stat, d_stat.p, sizeof stat, hipMemcpyDeviceToHost, stream));
    SW_HIP(hipStreamSynchronize(stream));
    const uint64_t max_threads = (uint64_t)launch_blocks(SQ_BLOCKS_ENV) * SQ_TPB;
    uint64_t launches = 0;
    for (uint32_t c = 0; c < LC_CLS_LDS; ++c) {   // register route, g = 2^c lanes per pair
        const uint64_t cnt = stat[c], g = 1ull << c, per_launch = std::max<uint64_t>(max_threads / g, 1);
        for (uint64_t x0 = 0; x0 < cnt; x0 += per_launch, ++launches) {
            a.list = lists.p + (uint64_t)c * n + x0;
            a.count = std::min<uint64_t>(per_launch, cnt - x0);
            a.g = (uint32_t)g;
            hipLaunchKernelGGL(k_lc, dim3(sq_blocks(a.count * g)), dim3(SQ_TPB), 0, stream, a);
            SW_HIP(hipGetLastError());
        }
    }
    DevArray<uint4> scratch;
    a.g = max_lanes;
    if (const uint64_t cnt = stat[LC_CLS_LDS]) {   // striped, the carry row in LDS: as long as the class's longest text
        const uint32_t groups = (uint32_t)std::min<uint64_t>({cnt, (uint64_t)LC_STRIPE_GROUPS, std::max<uint64_t>(max_threads / max_lanes, 1)});
        a.list = lists.p + (uint64_t)LC_CLS_LDS * n;
        a.count = cnt;
        hipLaunchKernelGGL(k_lc_striped<true>, dim3(groups), dim3(max_lanes), stat[10] * LC_CARRY_BYTES, stream, a);
        SW_HIP(hipGetLastError());
        ++launches;
    }
    if (const uint64_t cnt = stat[LC_CLS_HBM]) {   // striped, the carry row in HBM
        a.carry_stride = stat[11];
        const uint64_t fit = std::max<uint64_t>(LC_HBM_BYTES / (a.carry_stride * LC_CARRY_BYTES), 1);
        const uint32_t groups = (uint32_t)std::min<uint64_t>({cnt, (uint64_t)LC_STRIPE_GROUPS, std::max<uint64_t>(max_threads / max_lanes, 1), fit});
        scratch.alloc(2 * (uint64_t)groups * a.carry_stride);
        a.carry = scratch.p;
        a.list = lists.p + (uint64_t)LC_CLS_HBM * n;
        a.count = cnt;
        hipLaunchKernelGGL(k_lc_striped<false>, dim3(groups), dim3(max_lanes), 0, stream, a);
        SW_HIP(hipGetLastError());
        ++launches;
    }
    SW_HIP(hipEventRecord(e1, stream));
    SW_HIP(hipStreamSynchronize(stream));   // (lists / scratch go back to the pool behind the kernels)
    float ms = 0;
    SW_HIP(hipEventElapsedTime(&ms, e0, e1));
    st.ms[0] += ms;
    st.counters[0] += n;
    st.counters[1] += stat[9];
    st.counters[2] += stat[LC_CLS_LDS] + stat[LC_CLS_HBM];
    st.counters[3] += stat[LC_CLS_HBM];
    st.counters[4] += launches;
}

}  // namespace sw

using namespace sw;

extern "C" {

int sw_batch_local_alignments(const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs, uint64_t n,
                              const sw_scoring *scoring, uint32_t *score, uint32_t *qstart, uint32_t *qend, uint32_t *sstart, uint32_t *send, uint32_t *nident,
                              uint32_t *mismatch, uint32_t *gapopen, uint32_t *gaps, uint64_t *counters, double *ms)
{
    return guarded([&] {
        check_scoring("local alignments", scoring);
        check_infix_pairs("local alignments", b, offsets, blob, n_queries, pairs, n, true);
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t m = offsets[pairs[i].query + 1] - offsets[pairs[i].query], tn = pairs[i].stop - pairs[i].start;
            if (m >= (1ull << 16) || tn >= (1ull << 16))
                raise(SW_ERR_VALUE, "local alignments: pair %llu (a query of %llu bases, a text of %llu) reaches 2^16 on a side", (unsigned long long)i,
                      (unsigned long long)m, (unsigned long long)tn);
        }
        StreamScope scope(HIT_STREAM);
        DevRuns runs(*b);
        const uint64_t total = n_queries ? offsets[n_queries] : 0;
        DevArray<uint8_t> text(total);
        if (total) SW_HIP(hipMemcpyAsync(text.p, blob, total, hipMemcpyHostToDevice, HIT_STREAM));
        QueryPack P;
        pack_queries(text.p, offsets, n_queries, P);
        DevArray<sw_infix_pair> d_pairs(n);
        DevArray<uint32_t> d_out[LOCAL_FIELDS];
        uint32_t *out[LOCAL_FIELDS];
        for (uint32_t f = 0; f < LOCAL_FIELDS; ++f) {
            d_out[f].alloc(n);
            out[f] = d_out[f].p;
        }
        if (n) SW_HIP(hipMemcpyAsync(d_pairs.p, pairs, n * sizeof(sw_infix_pair), hipMemcpyHostToDevice, HIT_STREAM));
        LocalStats st;
        local_device(runs_of(runs.t), P, d_pairs.p, nullptr, n, *scoring, out, st);
        SW_HIP(hipStreamSynchronize(HIT_STREAM));
        uint32_t *const host[LOCAL_FIELDS] = {score, qstart, qend, sstart, send, nident, mismatch, gapopen, gaps};
        for (uint32_t f = 0; f < LOCAL_FIELDS; ++f)
            if (n && host[f]) SW_HIP(hipMemcpy(host[f], d_out[f].p, n * 4, hipMemcpyDeviceToHost));
        if (counters) memcpy(counters, st.counters, sizeof st.counters);
        if (ms) ms[0] = st.ms[0];
    });
}

static const sw_hits &local_of(const sw_hits *h)
{
    if (!h) raise(SW_ERR_VALUE, "best hits: a NULL handle");
    if (!h->has_local) raise(SW_ERR_VALUE, "best hits: these hits were made without the local alignment (sw_batch_best_hits_local makes it)");
    return *h;
}

int sw_hits_local_block(const sw_hits *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out)
{
    return guarded([&] {
        local_of(h);
        if (field >= LOCAL_FIELDS)
            raise(SW_ERR_VALUE, "best hits: field %llu is none of score, qstart, qend, sstart, send, nident, mismatch, gapopen, gaps (0..8)", (unsigned long long)field);
        export_cells("best hits", "queries", h->device, "the hits", h->lfield[field].p, h->nq, h->n_asm, r0, r1, c0, c1, out);
    });
}

int sw_hits_loci_local(const sw_hits *h, uint32_t *score, uint32_t *qstart, uint32_t *qend, uint32_t *sstart, uint32_t *send, uint32_t *nident, uint32_t *mismatch,
                       uint32_t *gapopen, uint32_t *gaps)
{
    return guarded([&] {
        local_of(h);
        if (!h->has_loci) raise(SW_ERR_VALUE, "best hits: these hits were made without the loci (sw_batch_best_hits_loci makes them)");
        require_device(h->device, "the hits");
        uint32_t *const out[LOCAL_FIELDS] = {score, qstart, qend, sstart, send, nident, mismatch, gapopen, gaps};
        for (uint32_t f = 0; f < LOCAL_FIELDS; ++f)
            if (out[f] && h->loci.n) SW_HIP(hipMemcpy(out[f], h->loci.lf[f].p, h->loci.n * 4, hipMemcpyDeviceToHost));
    });
}

int sw_hits_local_stats(const sw_hits *h, uint64_t *counters, double *ms)
{
    return guarded([&] {
        const sw_hits &x = local_of(h);
        if (counters) memcpy(counters, x.local.counters, sizeof x.local.counters);
        if (ms) ms[0] = x.local.ms[0];
    });
}

}  // extern "C"
