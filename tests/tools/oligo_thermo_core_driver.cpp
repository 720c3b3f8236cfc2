// Host driver of seqwin_amd/csrc/oligo_thermo_core.hpp: what k_ol_scan<true> does with a hit and what a thread of k_ol_thermo_best and
// of k_ol_thermo_sites does with a window, run on the CPU exactly as the kernels call it (tests/test_oligo_thermo_cpu.py, under
// AddressSanitizer + UBSan where g++ has them).
// stdin: the model -- 768 stack entries, 96 end entries, 3 of init, as decimal integers -- and then one case per line,
// `window oligo strand off`: the L bases of the text at a site over ACGT, an IUPAC oligo of L letters, the strand, and the batch-wide
// index of the window's first base.  stdout per case: `dh ds dg dg_alone mm` -- dg_alone from the form the scan kernel uses.
#include <cstdio>
#include <cstring>
#include <vector>

#include "oligo_thermo_core.hpp"

using namespace sw::olt;

static uint32_t iupac(char c)
{
    static const char *letters = "acgturyswkmbdhvn";
    static const uint32_t sets[] = {1, 2, 4, 8, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15};
    const char *p = strchr(letters, c | 0x20);
    return p ? sets[p - letters] : 0;
}

static uint32_t complement_set(uint32_t s)
{
    return ((s & 1) << 3) | ((s & 2) << 1) | ((s & 4) >> 1) | ((s & 8) >> 3);
}

int main()
{
    std::vector<int16_t> stack(STACK_WORDS), end(END_WORDS);   // (exactly the tables: a read beyond them is reported)
    Tables T{stack.data(), end.data(), {0, 0, 0}};
    int v;
    for (uint32_t i = 0; i < STACK_WORDS; ++i) {
        if (scanf("%d", &v) != 1) return 2;
        stack[i] = (int16_t)v;
    }
    for (uint32_t i = 0; i < END_WORDS; ++i) {
        if (scanf("%d", &v) != 1) return 2;
        end[i] = (int16_t)v;
    }
    for (uint32_t i = 0; i < PLANES; ++i)
        if (scanf("%d", &T.init[i]) != 1) return 2;
    char text[64], oligo[64];
    unsigned strand;
    unsigned long long off;
    while (scanf("%63s %63s %u %llu", text, oligo, &strand, &off) == 4) {
        const uint32_t L = (uint32_t)strlen(oligo);
        if (strlen(text) != L || L < 8 || L > 32 || strand > 1) return 3;
        // the packed words from the one that holds base `off` on (the driver's word 0), and no word more than the window needs
        const uint64_t w0 = off >> 4, words = ((off + L - 1) >> 4) - w0 + 1;
        std::vector<uint32_t> packed(words, 0xA5A5A5A5u);
        for (uint32_t j = 0; j < L; ++j) {
            const uint64_t x = off + j;
            const uint32_t code = (uint32_t)(strchr("ACGT", text[j]) - "ACGT");
            uint32_t &w = packed[(x >> 4) - w0];
            w = (w & ~(3u << (2 * (x & 15)))) | (code << (2 * (x & 15)));
        }
        uint32_t n[4] = {0, 0, 0, 0};   // the row of oligo.hip's pattern_rows on this strand
        for (uint32_t t = 0; t < L; ++t) {
            const uint32_t s = strand ? complement_set(iupac(oligo[t])) : iupac(oligo[L - 1 - t]);
            for (uint32_t b = 0; b < 4; ++b)
                if (!((s >> b) & 1)) n[b] |= 1u << t;
        }
        uint32_t lo, hi;
        window(packed.data(), off - (w0 << 4), L, lo, hi);   // (the same place in its word as in the batch)
        const Sums all = site<true>(lo, hi, n[0], n[1], n[2], n[3], L, strand, T);
        const Sums dg = site<false>(lo, hi, n[0], n[1], n[2], n[3], L, strand, T);
        const uint32_t mm = (uint32_t)__builtin_popcount(mismatches(lo, hi, n[0], n[1], n[2], n[3]));
        printf("%d %d %d %d %u\n", all.dh, all.ds, all.dg, dg.dg, mm);
    }
    return 0;
}
