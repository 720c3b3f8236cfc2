// seqs_core.hpp -- what seqs.hip and hits.hip share of the interval and edit-distance code: the batch as the kernels read it (RunTable,
// DevRuns), the interval check, the packed-base and validity loads, and one column of Myers' recurrence on a 64-row block.
// Device functions cannot be linked across translation units here, so both files include this header.
#pragma once
#include <cstring>  // rocprim's texture iterator needs ::memset declared first
#include <memory>

#include <rocprim/rocprim.hpp>

#include "device.hpp"

namespace sw {
namespace {

constexpr uint32_t SQ_TPB = 256, SQ_WAVE = 64, SQ_WPB = SQ_TPB / SQ_WAVE;
constexpr uint64_t SQ_MAX_LIST = 0xFFFFFF00ull; // most entries of a list: a thread per entry in workgroups of 256 stays below 2^32 threads
constexpr uint32_t SQ_PER_WAVE = 16;           // intervals a wave of k_fetch takes at most in one launch (grid stride)
constexpr uint32_t ED_CAP = 64;                // pattern blocks of the register route: the lanes of a wave (4096 bases)
constexpr uint32_t ED_CLASSES = 8;             // group widths 1, 2, ... 64, then the striped route
constexpr uint32_t ED_STRIPE_GROUPS = 1024;    // groups of a launch of the striped route (each owns one row of the scratch)

// workgroups per launch: launch_blocks(SQ_BLOCKS_ENV); the switch (test library) lowers it so that a small list needs several launches
constexpr const char *SQ_BLOCKS_ENV = "SEQWIN_AMD_SEQ_MAX_BLOCKS";

// pattern blocks up to which a pair stays on the register route; SEQWIN_AMD_DIST_LDS_CAP (test library) lowers it
uint32_t ed_cap_blocks()
{
    return (uint32_t)std::max<uint64_t>(std::min<uint64_t>(env_u64(SW_TEST_GETENV("SEQWIN_AMD_DIST_LDS_CAP"), ED_CAP), ED_CAP), 1);
}

struct RunTable {   // the batch as the kernels read it
    const uint32_t *packed;        // 16 bases per word, base i in bits [2 (i % 16), +2)
    const uint64_t *rec_base;      // [R] batch-wide index of the record's first base
    const uint32_t *rec_len;       // [R]
    const uint32_t *rec_run_off;   // [R + 1] the record's valid runs: [rec_run_off[r], rec_run_off[r + 1])
    const uint32_t *run_pos, *run_len;
    uint64_t n_records;
};

// ---- interval checks ------------------------------------------------------------------------------------------------------------
__global__ void k_iv_check(RunTable t, const sw_interval *iv, uint64_t n, unsigned long long *first_bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const sw_interval v = iv[i];
    if (v.record >= t.n_records || v.start > v.stop || v.stop > t.rec_len[v.record]) atomicMin(first_bad, (unsigned long long)i);
}


// first run of record r that ends behind position p (q1 of the record: none)
__device__ __forceinline__ uint32_t run_behind(const RunTable &t, uint32_t q0, uint32_t q1, uint32_t p)
{
    uint32_t lo = q0, hi = q1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)t.run_pos[mid] + t.run_len[mid] > p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---- edit distances -------------------------------------------------------------------------------------------------------------
// codes of bases [gp, gp + cnt) of the packed stream, cnt in 1..32, base i in bits [2i, 2i + 2); only the words that hold them are read
__device__ __forceinline__ uint64_t load_codes(const uint32_t *__restrict__ packed, uint64_t gp, uint32_t cnt)
{
    const uint64_t w = gp >> 4, last = (gp + cnt - 1) >> 4;
    const uint32_t sh = 2 * (uint32_t)(gp & 15);
    uint64_t x = packed[w];
    if (last > w) x |= (uint64_t)packed[w + 1] << 32;
    x >>= sh;
    if (last > w + 1) x |= (uint64_t)packed[w + 2] << (64 - sh);   // (then sh > 0)
    return x;
}

// A valid run [lo, hi) of record rec that a lane met before (none: lo == hi).  Run positions are relative to their record, so a
// remembered run answers for that record only.
struct RunMemo {
    uint32_t rec = 0, lo = 0, hi = 0;
};

// bit i set: base p + i of record rec is valid, i < cnt <= 32
__device__ uint32_t valid32(const RunTable &t, uint32_t rec, uint32_t p, uint32_t cnt, RunMemo &c)
{
    if (cnt == 0) return 0;
    const uint64_t end = (uint64_t)p + cnt;
    if (c.rec == rec && p >= c.lo && end <= c.hi) return cnt >= 32 ? 0xFFFFFFFFu : (1u << cnt) - 1;
    const uint32_t q1 = t.rec_run_off[rec + 1];
    uint32_t mask = 0;
    for (uint32_t q = run_behind(t, t.rec_run_off[rec], q1, p); q < q1; ++q) {
        const uint64_t a = t.run_pos[q], e = a + t.run_len[q];
        if (a >= end) break;
        const uint32_t x = (uint32_t)((a > p ? a : p) - p), y = (uint32_t)((e < end ? e : end) - p);   // 0 <= x < y <= cnt
        mask |= (y >= 32 ? 0xFFFFFFFFu : (1u << y) - 1) & ~((1u << x) - 1);
        c.rec = rec;
        c.lo = (uint32_t)a;
        c.hi = (uint32_t)e;
    }
    return mask;
}

// the even bits of x, packed
__device__ __forceinline__ uint32_t even_bits(uint64_t x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)x;
}

// One column of one 64-row block.  Horizontal deltas are coded 0: 0, 1: +1, 2: -1.  eq: rows that match the column's base.
__device__ __forceinline__ uint32_t myers_step(uint64_t eq, uint64_t &Pv, uint64_t &Mv, uint32_t hin, uint32_t out_bit)
{
    const uint64_t neg = hin == 2 ? 1ull : 0ull, pos = hin == 1 ? 1ull : 0ull;
    const uint64_t Xv = eq | Mv;
    eq |= neg;
    const uint64_t Xh = (((eq & Pv) + Pv) ^ Pv) | eq;
    uint64_t Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
    const uint32_t hout = ((Ph >> out_bit) & 1ull) ? 1u : ((Mh >> out_bit) & 1ull) ? 2u : 0u;
    Ph = (Ph << 1) | pos;
    Mh = (Mh << 1) | neg;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
    return hout;
}

constexpr hipStream_t SQ_STREAM = 0;

uint32_t sq_blocks(uint64_t n) { return (uint32_t)((n + SQ_TPB - 1) / SQ_TPB); }

// the run table of a batch on the device, uploaded once per call
struct DevRuns {
    DevArray<uint32_t> rec_len, rec_run_off, run_pos, run_len;
    RunTable t{};
    explicit DevRuns(const sw_batch &b)
    {
        const HostBatch &h = b.host;
        const size_t R = h.rec_len.size(), Q = h.run_pos.size();
        if (R != b.n_records || h.rec_run_off.size() != R + 1 || h.run_len.size() != Q || (R && h.rec_run_off[R] != Q))
            raise(SW_ERR_RUNTIME, "the batch's run table does not describe its %llu records", (unsigned long long)b.n_records);
        if (R && (!b.d_packed.p || !b.d_rec_base.p)) raise(SW_ERR_VALUE, "the batch holds no packed bases (it must be resident)");
        rec_len.alloc(R);
        rec_run_off.alloc(R + 1);
        run_pos.alloc(Q);
        run_len.alloc(Q);
        auto up = [&](void *dst, const void *src, size_t bytes) {
            if (bytes) SW_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, SQ_STREAM));
        };
        up(rec_len.p, h.rec_len.data(), R * 4);
        up(rec_run_off.p, h.rec_run_off.data(), (R + 1) * 4);
        up(run_pos.p, h.run_pos.data(), Q * 4);
        up(run_len.p, h.run_len.data(), Q * 4);
        t = RunTable{b.d_packed.p, b.d_rec_base.p, rec_len.p, rec_run_off.p, run_pos.p, run_len.p, (uint64_t)R};
    }
};

// SW_ERR_VALUE naming the first interval of the device list that does not lie in its record
void check_intervals(const RunTable &t, const sw_interval *d_iv, uint64_t n, const char *what)
{
    if (!n) return;
    if (n > SQ_MAX_LIST) raise(SW_ERR_VALUE, "%s: %llu intervals exceed one launch of the list kernels (%llu)", what, (unsigned long long)n, (unsigned long long)SQ_MAX_LIST);
    DevArray<unsigned long long> bad(1);
    SW_HIP(hipMemsetAsync(bad.p, 0xFF, 8, SQ_STREAM));
    hipLaunchKernelGGL(k_iv_check, dim3(sq_blocks(n)), dim3(SQ_TPB), 0, SQ_STREAM, t, d_iv, n, bad.p);   // (n <= SQ_MAX_LIST: below 2^32 threads)
    SW_HIP(hipGetLastError());
    unsigned long long first = 0;
    SW_HIP(hipMemcpy(&first, bad.p, 8, hipMemcpyDeviceToHost));
    if (first == ~0ull) return;
    sw_interval v{};
    SW_HIP(hipMemcpy(&v, d_iv + first, sizeof v, hipMemcpyDeviceToHost));
    raise(SW_ERR_VALUE, "%s: interval %llu (record %u, [%u, %u)) does not lie inside one of the batch's %llu records", what, first, v.record, v.start,
          v.stop, (unsigned long long)t.n_records);
}

}  // namespace
}  // namespace sw
