// Host driver of seqwin_amd/csrc/oligo_edit_core.hpp: what a lane of k_ole_scan and a thread of k_ole_resolve compute, run on the CPU
// exactly as the kernels call it (tests/test_oligo_edit_cpu.py, under AddressSanitizer + UBSan where g++ has them).
// stdin: one case per line, `text oligo d c k off` -- a run over ACGT, an IUPAC oligo, max_edits, three_prime, the tiles' k (Lmin - d)
// and the run's batch-wide base index.  stdout: `case i` and then one line `strand pos end dist mismatch gaps` per site, lane by lane.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "oligo_edit_core.hpp"

using namespace sw::ole;

static uint32_t iupac(char c)
{
    static const char *letters = "acgturyswkmbdhvn";
    static const uint32_t sets[] = {1, 2, 4, 8, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15};
    const char *p = strchr(letters, c | 0x20);
    return p ? sets[p - letters] : 0;
}

int main()
{
    char text[8192], oligo[64];
    unsigned d, c, k, off;
    for (int i = 0; scanf("%8191s %63s %u %u %u %u", text, oligo, &d, &c, &k, &off) == 6; ++i) {
        const uint32_t n = (uint32_t)strlen(text), L = (uint32_t)strlen(oligo);
        std::vector<uint32_t> packed((n + off) / 16 + 1, 0xA5A5A5A5u);   // (exactly the words that hold the run: a read beyond them is reported)
        for (uint32_t j = 0; j < n; ++j) {
            const uint64_t x = (uint64_t)off + j;
            const uint32_t code = (uint32_t)(strchr("ACGT", text[j]) - "ACGT");
            packed[x >> 4] = (packed[x >> 4] & ~(3u << (2 * (x & 15)))) | (code << (2 * (x & 15)));
        }
        uint32_t eq[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < L; ++j)
            for (uint32_t b = 0; b < 4; ++b)
                if ((iupac(oligo[j]) >> b) & 1) eq[b] |= 1u << j;
        printf("case %d\n", i);
        if (n < k) continue;
        const uint32_t nk = n - k + 1;
        for (uint32_t first = 0; first < nk; first += 16) {              // a lane's 16 places
            const uint32_t cnt = nk - first < 16 ? nk - first : 16;
            for (uint32_t s = 0; s < 2; ++s) {
                const uint32_t a = first_end(s, n, k, first, cnt);
                const OleStream st = load_stream(packed.data(), off, n, s, a, cnt, d);
                const uint32_t cand = ole_scan(st, a, cnt, n, d, c, L, eq[0], eq[1], eq[2], eq[3]);
                for (uint32_t x = 0; x < cnt; ++x) {
                    if (!((cand >> x) & 1)) continue;
                    const uint32_t e = a + x;
                    const OleSite r = ole_align(packed.data(), off, n, s, e, d, c, L, eq);
                    printf("%u %u %u %u %u %u\n", s, s ? n - e : r.b, s ? n - r.b : e, r.dist, r.mismatch, r.gaps);
                }
            }
        }
    }
    return 0;
}
