// oligo_result.hpp -- the result of an oligo search as its two readers see it: oligo.hip makes it and exports it, amplicons.hip reads
// the finished site list.  The layout of a site key is the part of it both need.
#pragma once
#include "device.hpp"

namespace sw {
// a site key keeps the oligo in its top bits; below it the batch-wide base index of pos, then
//   a Hamming result (oligo << 48):  strand << 4 | mm
//   an edit result   (oligo << 52):  (end - pos - (L - d)) << 5 | strand << 4 | code;  code = 5 t + mismatch, gaps = |end - pos - L| + 2 t
constexpr uint32_t OL_SITE_Q_SHIFT = 48, OLE_SITE_Q_SHIFT = 52;
}  // namespace sw

struct sw_oligos {
    int device = 0;
    uint64_t nq = 0, n_asm = 0, max_mm = 0, three_prime = 0;
    int64_t max_edits = -1;                // -1: a Hamming result
    std::vector<uint32_t> lens;            // [nq] the oligos' lengths
    sw::DevArray<uint32_t> field[8];       // [nq][n_asm] n_sites, best_mm (an edit result: best_dist), best_record, best_pos, best_strand;
                                           // an edit result only: best_end, best_mismatch, best_gaps
    bool has_sites = false;
    uint64_t n_list = 0;
    sw::DevArray<uint64_t> keys;           // [n_list] the site keys, ascending
    sw::DevArray<uint32_t> s_asm, s_rec, s_pos;
    uint64_t counters[8] = {};             // sw_oligos_stats
    double ms[2] = {};                     // scan, order
    uint64_t edit_counters[2] = {};        // sw_oligos_edit_stats: DP steps, candidates resolved
    double resolve_ms = 0;
    // a Hamming result made with a thermodynamic model (section 3.2o); nothing of it is allocated without one
    bool thermo = false;
    sw::DevArray<uint32_t> n_stable;       // [nq][n_asm]
    sw::DevArray<int32_t> stable_sum[3];   // [nq][n_asm] stable_dg, stable_dh, stable_ds
    sw::DevArray<uint32_t> stable_at[4];   // [nq][n_asm] stable_record, stable_pos, stable_strand, stable_mm
    sw::DevArray<int32_t> s_sum[3];        // [n_list] dh, ds, dg of the sites
    double thermo_ms[2] = {};              // k_ol_thermo_best, k_ol_thermo_sites
};
