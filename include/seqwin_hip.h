/*
 * seqwin_hip.h -- C ABI of libseqwin_hip.so, the MI355X (gfx950) implementation of Seqwin's
 * minimizer-index hot path.
 *
 * The entry points are exactly what the reference's native boundary for this path binds
 * (the pybind11 module `seqwin.graph._core`, cpp/src/bindings/python_bindings.cpp:43-169, over
 * cpp/include/seqwin/{build,filter,graph}.hpp); each declaration cites the reference interface it
 * replaces.  Plain pointers and sizes only -- no C++/torch types cross this boundary.
 *
 * Conventions
 *   - Every function returning `int` returns SW_OK or an SW_ERR_* code; the message is available
 *     from sw_last_error() (thread-local).  Code -> Python exception mapping mirrors pybind11's
 *     translation of the reference's C++ exceptions: SW_ERR_RUNTIME <- std::runtime_error /
 *     std::logic_error -> RuntimeError; SW_ERR_VALUE <- std::invalid_argument -> ValueError.
 *   - There is NO CPU fallback: if no HIP device is usable the calls fail with SW_ERR_DEVICE.
 *   - Wire formats are the reference's PODs, byte for byte (cpp/include/seqwin/graph.hpp:15-53):
 *     sw_kmer 8 B, sw_node 40 B, sw_edge 24 B.
 */
#ifndef SEQWIN_HIP_H
#define SEQWIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SW_OK 0
#define SW_ERR_RUNTIME 1 /* std::runtime_error / std::logic_error in the reference */
#define SW_ERR_VALUE 2   /* std::invalid_argument in the reference */
#define SW_ERR_DEVICE 3  /* no usable HIP device / HIP runtime error (no reference analogue) */

/* seqwin::Kmer, cpp/include/seqwin/graph.hpp:15-20 */
typedef struct sw_kmer {
    uint32_t pos;
    uint32_t record_idx;
} sw_kmer;

/* seqwin::Node, cpp/include/seqwin/graph.hpp:28-41 */
typedef struct sw_node {
    uint64_t hash;
    uint64_t start;
    uint64_t stop;
    uint32_t n_tar;
    uint32_t n_neg;
    double penalty;
} sw_node;

/* seqwin::Edge, cpp/include/seqwin/graph.hpp:46-53 */
typedef struct sw_edge {
    uint64_t first;
    uint64_t second;
    uint64_t weight;
} sw_edge;

typedef struct sw_graph sw_graph; /* opaque result of sw_build (host-resident arrays) */
typedef struct sw_batch sw_batch; /* opaque device-resident batch of 2-bit packed assemblies */
typedef struct sw_index sw_index; /* opaque device-resident index built from a batch */

/* ---- diagnostics -------------------------------------------------------------------------- */
const char *sw_last_error(void);
const char *sw_version(void);
/* Log sink (replaces log_python, cpp/src/utils/logging.cpp:9-29, which logs to Python's root logger from native code):
 * fn(level, message) with level in {"debug", "info", "warning", "error"} is called on the thread that called into the
 * library; NULL (the default) drops the messages.  sw_build reports one "info" line per call. */
typedef void (*sw_log_fn)(const char *level, const char *message);
void sw_set_log_callback(sw_log_fn fn);
/* Number of visible HIP devices (0 when none / runtime unusable). Does not initialise a context. */
int sw_device_count(void);
/* Select the HIP device used by the calling thread for all later calls (default 0). */
int sw_set_device(int device);

/* ---- drop-in entry points (host arrays in, host arrays out) ------------------------------- */

/*
 * Replaces `_build_native(assembly_paths, kmerlen, windowsize, n_cpu, low_memory)`
 * (python_bindings.cpp:50-90) = seqwin::build (cpp/include/seqwin/build.hpp:22-28,
 * cpp/src/seqwin/build.cpp:330-394).  FASTA/gz files are read and 2-bit packed on `n_cpu` host
 * threads, sketched and indexed on the GPU, and the result is copied back into *out.
 * `low_memory` (build.cpp:264-325: the reference recomputes the sketches in a second pass to keep the peak down) streams the
 * assemblies through HBM in consecutive chunks of SEQWIN_AMD_LOWMEM_CHUNK_MBP Mbp (default 4096): only 24 B per
 * minimizer of a finished chunk stay resident, and the index is built once from the concatenated tuple stream -- results are
 * identical either way (reference tests/smoke/test_graph.py:222-245).  The same route is taken without the flag when the
 * files exceed SEQWIN_AMD_HBM_BUDGET_GB (if set).
 * Any windowsize >= 1 is taken (minimizer.cpp:53-90 has no upper limit either; a window longer than a record's k-mers
 * gives no minimizer for it, :56-58).
 * Errors: k < 3, k > 65535, w < 1 -> SW_ERR_VALUE; unreadable file, FASTA
 * without header, > 2^32-1 records or bases per record -> SW_ERR_RUNTIME (build.cpp:136-147,337-339;
 * fasta_reader.cpp:69-71,99-102).
 */
int sw_build(const char *const *assembly_paths, size_t n_assemblies, uint64_t kmerlen, uint64_t windowsize,
             uint64_t n_cpu, int low_memory, sw_graph **out);

/* Sizes of the arrays held by a graph (the shapes `_build_native` returns). `ids_bytes` is the size of
 * the NUL-separated record-id blob (one id per FASTA record, in global record order). */
int sw_graph_sizes(const sw_graph *g, uint64_t *n_kmers, uint64_t *n_nodes, uint64_t *n_edges,
                   uint64_t *n_assemblies, uint64_t *ids_bytes, uint64_t *total_bp);

/* Copy the graph into caller-owned buffers (numpy arrays allocated by the Python glue):
 * kmers[n_kmers], nodes[n_nodes] (n_tar = n_neg = 0, penalty = 0.0), edges[n_edges],
 * record_offsets[n_assemblies + 1], ids_blob[ids_bytes].  Replaces array_to_numpy
 * (python_bindings.cpp:21-39, 69-83) without foreign-owned memory outliving the call.  (Large results cross PCIe through a
 * ring of pinned slots, nodes and edges in a packed form that host threads expand into these buffers: same bytes.) */
int sw_graph_export(const sw_graph *g, sw_kmer *kmers, sw_node *nodes, sw_edge *edges,
                    uint32_t *record_offsets, char *ids_blob);
/* Where the time of the sw_build that made g (and of its sw_graph_export) went, in ms: out[0] ingest + upload (host parse and
 * 2-bit packing with the pipelined copy to HBM), [1] the device part (wall), [2] launch plan, [3] sketch kernel, [4] tuple
 * order, [5] nodes stage, [6] edges stage, [7] sw_graph_export (0 before it ran). */
int sw_graph_stats(const sw_graph *g, double *out8);

/* Frees the graph handle.  The device index of an EXPORTED graph stays resident (one per process, replaced by the next
 * sw_build): sw_get_penalty / sw_filter_kmers work on it instead of uploading the caller's arrays again when those are
 * still the exported ones (same sizes and position-dependent checksums, verified on the host).  sw_release_resident()
 * gives that HBM back at once; SEQWIN_AMD_NO_RESIDENT=1 disables the mechanism. */
void sw_graph_free(sw_graph *g);
void sw_release_resident(void);
/* Device memory comes from a caching pool (steady-state builds do no hipMalloc).  sw_pool_trim() hands every cached, unused
 * block back to the driver -- for a host program that shares the GPU's memory with another allocator (torch's, in the
 * multi-GPU choreography); the pool trims itself when one of its own hipMalloc calls fails.  HOST memory the library keeps for
 * the life of the process: the page-locked rings of the up- and download (32 + 64 MiB per device) and the page-locked blocks the
 * streaming ingest packs into (grown on demand to at most SEQWIN_AMD_PINNED_POOL_MB, default 1024; 0 disables them). */
void sw_pool_trim(void);
/* out[3] = { 1 if SEQWIN_AMD_POOL_DEBUG is on (every release waits for the device and poisons the block, every reuse waits and
 * checks the poison: a soak mode for the multi-device path), blocks found written after their release, host-side hand-overs of
 * a block between threads / streams so far (0 in single-stream builds) } */
void sw_pool_debug_stats(uint64_t *out);
/* out[3] = { occurrences of the resident index (0: none), sw_get_penalty calls served from it, sw_filter_kmers calls served from it } */
void sw_resident_stats(uint64_t *out);

/*
 * Replaces `_get_penalty_native(kmers, nodes, record_offsets, is_targets, n_cpu)`
 * (python_bindings.cpp:92-135) = seqwin::get_penalty (cpp/include/seqwin/filter.hpp:11-20,
 * cpp/src/seqwin/filter.cpp:15-137).  Mutates nodes[].{n_tar,n_neg,penalty} in place.
 * Unlike the reference, the kmers length is passed and node ranges are checked against it.
 * All validation failures are SW_ERR_VALUE with the reference's messages (filter.cpp:33-60,103-123).
 */
int sw_get_penalty(const sw_kmer *kmers, uint64_t n_kmers, sw_node *nodes, uint64_t n_nodes,
                   const uint32_t *record_offsets, uint64_t n_record_offsets, const uint8_t *is_targets,
                   uint64_t n_assemblies, uint64_t n_cpu);

/*
 * Replaces `_filter_kmers_native(kmers, nodes, used_hashes)` (python_bindings.cpp:137-168) =
 * seqwin::filter_kmers (cpp/src/seqwin/filter.cpp:139-201).  Two-phase: call with kmers_out ==
 * nodes_out == NULL to obtain the output sizes, then again with buffers of those sizes; the second call of the same
 * thread with the same arguments only copies the result of the first out (one upload, one compute per pair).
 */
int sw_filter_kmers(const sw_kmer *kmers, uint64_t n_kmers, const sw_node *nodes, uint64_t n_nodes,
                    const uint64_t *used_hashes, uint64_t n_used, sw_kmer *kmers_out, sw_node *nodes_out,
                    uint64_t *n_kmers_out, uint64_t *n_nodes_out);

/* ---- host ingest only (no GPU needed; used by the CPU test-suite to check the FASTA reader / packer) */
typedef struct sw_hostbatch sw_hostbatch;
/* Read + 2-bit pack FASTA / .gz files exactly as sw_build / sw_batch_from_fasta do
 * (replaces read_fasta, cpp/src/utils/fasta_reader.cpp:207-213), without uploading. */
int sw_host_ingest(const char *const *assembly_paths, size_t n_assemblies, uint64_t n_cpu, sw_hostbatch **out);
int sw_hostbatch_info(const sw_hostbatch *hb, uint64_t *n_assemblies, uint64_t *n_records, uint64_t *total_bp,
                      uint64_t *ids_bytes, uint64_t *n_runs);
/* record_offsets[n_assemblies + 1], ids blob, rec_len[n_records] (any may be NULL) */
int sw_hostbatch_tables(const sw_hostbatch *hb, uint32_t *record_offsets, char *ids_blob, uint32_t *rec_len);
/* Decode record `record_idx` back to ASCII (A/C/G/T; 'N' for every invalid base). */
int sw_hostbatch_record(const sw_hostbatch *hb, uint64_t record_idx, char *seq_out, uint64_t cap, uint64_t *len_out);
void sw_hostbatch_free(sw_hostbatch *hb);

/* ---- device-resident pipeline (what sw_build is made of; used by bench.py and multi-GPU) --- */

#define SW_MAX_WINDOW 4096u   /* largest window the tile kernels take directly */
#define SW_WINDOW_SPLIT 2048u /* windows above this are sketched with w' = 1024 and selected from that superset (sketch.hip: get_plan) */

/* Host ingest: read + pack FASTA files (fasta_reader.cpp:207-213 semantics) on n_cpu host threads and upload them
 * as one device-resident batch (assembly i of the batch = assembly_paths[i]). */
int sw_batch_from_fasta(const char *const *assembly_paths, size_t n_assemblies, uint64_t n_cpu, sw_batch **out);
/* Inputs that are all single-member .gz files and number 320 per host thread or more (SEQWIN_AMD_DEVICE_INFLATE=1: any number, =0: never)
 * are inflated, parsed and packed ON THE DEVICE (the gzip branch of fasta_reader.cpp:109-203 and the parse of :41-95, one
 * file per lane; csrc/ingest_dev.hip) -- same batch, bit for bit; anything irregular in a file sends the whole call through
 * the host route, which reports errors the way the reference does.  Number of batches this process built that way: */
uint64_t sw_device_gz_batches(void);

/* Synthetic batch generated ON DEVICE: n_genomes assemblies x records_per_genome records of
 * `record_len` bases each, derived from `n_ancestors` iid-uniform ancestors with per-base
 * substitution probability snp_ppm / 1e6 (counter-based RNG, `seed`).  No host ingest. */
int sw_batch_synthetic(uint64_t n_genomes, uint64_t records_per_genome, uint64_t record_len,
                       uint64_t n_ancestors, uint64_t snp_ppm, uint64_t seed, sw_batch **out);
/* Genomes [first_genome, first_genome + n_genomes) of the same job: bases and record ids are those the unsharded
 * batch holds for these genomes (one rank's contiguous assembly range, cpp/src/seqwin/build.cpp:350-356). */
int sw_batch_synthetic_shard(uint64_t n_genomes, uint64_t records_per_genome, uint64_t record_len,
                             uint64_t n_ancestors, uint64_t snp_ppm, uint64_t seed, uint64_t first_genome,
                             sw_batch **out);

/* Ragged draft assemblies for the measurements (r06): genome g of the job has 20 ... 300 contigs whose lengths follow a bell over
 * 200 bp ... 1.5 Mbp (200 * 2^x, x a sum of four uniforms; median ~17 kbp) until ~genome_bp bases are reached, cut from ancestor
 * g % n_ancestors with snp_ppm substitutions; one contig in ten carries one to three scaffold gaps of 10 ... 1000 N.  The shape of
 * real inputs (tests/targets.txt assemblies): short-record tiles, gap tiles and the generic kernel's list mode at scale. */
int sw_batch_synthetic_ragged(uint64_t n_genomes, uint64_t genome_bp, uint64_t n_ancestors, uint64_t snp_ppm, uint64_t seed, uint64_t first_genome,
                              sw_batch **out);
/* Copy the ASCII sequence of record `record_idx` (A/C/G/T, 'N' for invalid bases) back to the host;
 * used by tests to hand the same input to the oracle. *len_out receives the record length. */
int sw_batch_record(const sw_batch *b, uint64_t record_idx, char *seq_out, uint64_t cap, uint64_t *len_out);
/* Assemblies [first_assembly, first_assembly + n_assemblies) of a batch as plain FASTA files <dir>/g<global index>.fa (ids as
 * ingested, sequence lines of line_width bases, 0 = one line per record; bases outside the valid runs are written as N),
 * decoded from HBM by n_cpu host threads.  Tooling for the benchmarks and tests that feed a device-generated batch to the
 * FASTA boundary and to the CPU reference. */
int sw_batch_write_fasta(const sw_batch *b, uint64_t first_assembly, uint64_t n_assemblies, const char *dir, uint64_t n_cpu,
                         uint64_t line_width);

int sw_batch_info(const sw_batch *b, uint64_t *n_assemblies, uint64_t *n_records, uint64_t *total_bp,
                  uint64_t *device_bytes);
/* record_offsets[n_assemblies + 1] and the NUL-separated id blob of a batch. */
int sw_batch_records(const sw_batch *b, uint32_t *record_offsets, char *ids_blob, uint64_t ids_cap,
                     uint64_t *ids_bytes);
void sw_batch_free(sw_batch *b);

/* Timings of the last sw_index_build on this index, in milliseconds (HIP events on the build stream). */
typedef struct sw_timings {
    double total_ms;
    double sketch_ms;    /* the fused ntHash + window-minimum kernel (dominant kernel) */
    double order_ms;     /* tile-order compaction of the tuple stream */
    double nodes_ms;     /* radix sort by hash + run-length -> nodes / kmers / ranks */
    double counts_ms;    /* per-node target / non-target assembly counts + penalty (side stream, overlaps edges_ms) */
    double edges_ms;     /* adjacency pairs -> sort -> weights */
    uint64_t sketch_launches;
    uint64_t n_tiles;
    uint64_t total_bp;
    uint64_t n_windows;
    uint64_t ovf_tiles;  /* fast-class tiles done by the generic kernel's list pass: tiles crossing invalid bases + tiles with more suffix records than published */
    double plan_ms;      /* host + upload time the (batch, k, w) launch plan took when it was built (tile tables, roll LUTs);
                            cached in the batch afterwards, so it is outside total_ms except for the first build */
    uint64_t plan_cached; /* 1: this build found the plan in the batch's cache */
    /* r06: the plan's tiles by class -- fast kernel with 256-thread / 64-thread workgroups, generic kernel (records that are mostly
     * gaps, w < 4, k > 256), and the fast-class tiles that cross an invalid-base gap (done by the generic kernel's list mode) */
    uint64_t tiles_b256, tiles_b64, tiles_generic, tiles_gap;
} sw_timings;

/*
 * Build the index of a resident batch: sketch (ntHash + windowed minimizers, nthash_kmer.hpp /
 * minimizer.cpp:53-90) -> nodes/kmers (build.cpp:153-253, build_internals.cpp:159-251) ->
 * edges (build.cpp:177-189, build_internals.cpp:253-291) -> if is_targets != NULL, per-node
 * counts and penalty (filter.cpp:62-136).  Everything stays in HBM; `stream` is a hipStream_t
 * (0 = default stream).  The call is asynchronous only up to internal size read-backs.
 */
int sw_index_build(const sw_batch *b, uint64_t kmerlen, uint64_t windowsize, const uint8_t *is_targets,
                   uint64_t n_assemblies, void *stream, sw_index **out);

int sw_index_sizes(const sw_index *ix, uint64_t *n_kmers, uint64_t *n_nodes, uint64_t *n_edges);
int sw_index_timings(const sw_index *ix, sw_timings *t);
/* D2H copies of the final arrays (any pointer may be NULL to skip that array). */
int sw_index_export(const sw_index *ix, sw_kmer *kmers, sw_node *nodes, sw_edge *edges);
/* 64-bit checksums of the three arrays (sum over elements of a mix of the element and its index, so order matters),
 * computed on device; seqwin_amd.device.host_checksums is the numpy restatement. */
int sw_index_checksums(const sw_index *ix, uint64_t *kmers_sum, uint64_t *nodes_sum, uint64_t *edges_sum);
/* The same for one rank's slice of a sharded index: element i of the slice counts as element base + i of the
 * concatenated arrays, so the sums of all slices add up (mod 2^64) to the checksums of the unsharded index --
 * shard-count invariance (reference tests/smoke/test_graph.py:67-127) checked without gathering.  sums[3]. */
int sw_index_checksums_at(const sw_index *ix, uint64_t kmer_base, uint64_t node_base, uint64_t edge_base, uint64_t *sums);
/* Self-check of a resident index on the device -- the size-independent properties of the reference's output, for sets
 * too large to compare on the host.  out[10]: numbers of violations [0] nodes strictly ascending by hash
 * (build_internals.cpp:220), [1] node ranges partition the occurrences (:203-218), [2] (record_idx, pos) strictly ascending
 * inside a node (build.cpp:232-240), [3] edges strictly ascending by (first, second) (build_internals.cpp:261),
 * [4] first <= second, [5] 1 <= weight <= n_assemblies (build.cpp:177-189), [6] edge endpoints are node hashes,
 * [7] (scored != 0) 1 <= n_tar + n_neg <= min(node size, n_assemblies) (filter.cpp:62-136); then [8] the sum of the
 * edge weights and [9] reserved.  All of [0..7] are 0 for a correct index. */
int sw_index_verify(const sw_index *ix, uint64_t n_assemblies, int scored, uint64_t *out);
/* The sketch stage alone: (out_hash, pos, record_idx) of every minimizer in (record_idx, pos) order.
 * Two-phase like sw_filter_kmers: pass NULL buffers to get *n_out. */
int sw_sketch(const sw_batch *b, uint64_t kmerlen, uint64_t windowsize, void *stream, uint64_t *out_hash,
              sw_kmer *kmers, uint64_t cap, uint64_t *n_out);
void sw_index_free(sw_index *ix);

/* ---- next rows of the path, device-resident: what kmers.filter_graph does with the arrays ------
 * sums[3] = { sum n_tar, sum n_tar^2, sum n_tar * n_neg } over the nodes: the exact integer sums behind the
 * minimizer-sketch penalty threshold (src/seqwin/kmers.py:426-429). */
int sw_index_threshold_sums(const sw_index *ix, uint64_t *sums);
/* kmers._filter_edges_and_nodes (src/seqwin/kmers.py:132-173) without leaving HBM: *out holds the edges with
 * weight > edge_weight_th (already floored, np.uintp(th)) and the nodes that are an endpoint of one; no kmers. */
int sw_index_filter_graph(const sw_index *ix, uint64_t edge_weight_th, sw_index **out);
/* seqwin::filter_kmers (filter.cpp:139-201) on a resident index: *out holds the nodes of `nodes_from` whose hash is
 * in used_hashes (host array) and their kmers (taken from `ix`), ranges re-based; no edges. */
int sw_index_filter_kmers(const sw_index *ix, const sw_index *nodes_from, const uint64_t *used_hashes, uint64_t n_used,
                          sw_index **out);

/* ---- kmers._get_subgraphs (src/seqwin/kmers.py:176-312) on the device (csrc/subgraph.hip) ---------------------------------
 * Greedy seed expansion of low-penalty subgraphs over a filtered index (sw_index_filter_graph, or sw_index_from_arrays).
 * Seeds are the nodes of the graph (endpoints of an edge) with penalty <= penalty_th in ascending hash order (kmers.py:237-246);
 * rng.shuffle depends on the list's length only, so the caller shuffles list(range(n_seeds)) and passes it as seed_perm
 * (shuffled seed i = seed seed_perm[i]).  The result is the reference's `subgraphs` in commit order (before its final
 * rng.shuffle, kmers.py:309, which the caller does the same way) and `used`.  Arithmetic in double, as the reference does it. */
typedef struct sw_subgraphs sw_subgraphs; /* opaque device-resident result of sw_index_subgraphs */
/* A filtered graph given as host arrays (what _filter_edges_and_nodes returns, kmers.py:132-173), uploaded as an index without
 * kmers: nodes strictly ascending by hash with finite non-negative penalties (SW_ERR_VALUE otherwise). */
int sw_index_from_arrays(const sw_node *nodes, uint64_t n_nodes, const sw_edge *edges, uint64_t n_edges, sw_index **out);
/* Number of seeds at penalty_th (kmers.py:243-245). */
int sw_index_subgraph_seeds(const sw_index *f, double penalty_th, uint64_t *n_seeds);
/* The walk (kmers.py:248-301).  max_nodes = UINT64_MAX for None.  seed_perm[n_seeds]: host array, a permutation of
 * 0 .. n_seeds - 1 (SW_ERR_VALUE otherwise, or if n_seeds is not the number of seeds).  Zero subgraphs is a result here; the
 * reference's RuntimeError (kmers.py:300-307) is raised by the caller. */
int sw_index_subgraphs(const sw_index *f, double penalty_th, uint64_t min_nodes, uint64_t max_nodes, const uint64_t *seed_perm,
                       uint64_t n_seeds, sw_subgraphs **out);
/* Sizes: subgraphs, their nodes (= |used|), induced edges, nodes of the filtered graph. */
int sw_subgraphs_sizes(const sw_subgraphs *sg, uint64_t *n_subgraphs, uint64_t *n_sg_nodes, uint64_t *n_induced_edges,
                       uint64_t *n_nodes);
/* D2H copies (any pointer may be NULL): offsets[n_subgraphs + 1] and hashes[n_sg_nodes] (ascending inside each subgraph), in
 * commit order; edge_offsets[n_subgraphs + 1] and edges[n_induced_edges]: the filtered edges with both endpoints in the same
 * subgraph (nx_graph.subgraph(sg), markers.py:418), grouped by subgraph, in edge order inside a group; used_mask[n_nodes] over
 * the filtered nodes; used_hashes[n_sg_nodes] ascending. */
int sw_subgraphs_export(const sw_subgraphs *sg, uint64_t *offsets, uint64_t *hashes, uint64_t *edge_offsets, sw_edge *edges,
                        uint8_t *used_mask, uint64_t *used_hashes);
/* counters[10] = { seeds, rounds, expansions run, expansions invalidated (re-run in a later round), seeds skipped as used,
 * kept expansions, discarded expansions (< min_nodes), largest frontier, spilled expansions, last window size };
 * ms[3] = { adjacency + seeds, walk, results } (HIP events). */
int sw_subgraphs_stats(const sw_subgraphs *sg, uint64_t *counters, double *ms);
void sw_subgraphs_free(sw_subgraphs *sg);
/* sw_index_filter_kmers with the subgraphs' used nodes (the device `used`, no host set): seqwin::filter_kmers
 * (filter.cpp:139-201) as kmers.py:113-116 calls it after the walk. */
int sw_index_filter_kmers_sg(const sw_index *ix, const sw_index *nodes_from, const sw_subgraphs *sg, sw_index **out);

/* ---- markers._get_cks' per-subgraph work (src/seqwin/markers.py:95-300, 356-426) on the device (csrc/markers.hip) ----------
 * For every subgraph: its location in every assembly (ConnectedKmers.__get_loc, markers.py:192-254) and its representative
 * k-mer ordering with the row that carries it (__get_rep_order, markers.py:256-299; `rep`, markers.py:160).
 * Items of a (subgraph, assembly) pair: the occurrences of the subgraph's nodes in the assembly's records, by (record_idx, pos).
 * A run of consecutive minimizers ends at a change of record and where 2 * (pos - previous pos) > 3 * windowsize
 * (pos.diff() > 1.5 * windowsize, markers.py:217, in integers).  A row describes the largest run of its assembly, the earliest
 * one on ties (idxmax, markers.py:240-244); assemblies without an item have no row; rows ascend by assembly.  Targets are the
 * assemblies below n_tar.  record_idx is local to the assembly, stop = last pos + kmerlen in uint32 as the reference's column. */
typedef struct sw_marker_row {
    uint32_t assembly_idx;
    uint32_t record_idx;
    uint32_t start;
    uint32_t stop;
    uint32_t n_kmers;
    uint32_t n_repeats; /* runs of the subgraph in this assembly */
} sw_marker_row;
#define SW_MARKER_SINGLE 1u    /* the representative ordering has one k-mer (markers.py:294-295) */
#define SW_MARKER_DUP 2u       /* a hash occurs twice in it (markers.py:296-297) */
#define SW_MARKER_NO_TARGET 4u /* no target assembly holds the subgraph: the reference raises ValueError (max of an empty sequence, markers.py:283) */
typedef struct sw_marker_rep {
    sw_marker_row row; /* the lowest-assembly row whose ordering is the representative one (markers.py:160) */
    uint32_t n_rep;    /* target rows with the representative's canonical ordering (markers.py:299); 0 with SW_MARKER_NO_TARGET */
    uint32_t flags;
} sw_marker_rep;
typedef struct sw_markers sw_markers; /* opaque device-resident result */
/* The resident route: kept = the index of sw_index_filter_kmers_sg, sg = the walk's result; subgraphs in commit order.
 * record_offsets[n_assemblies + 1] (host) must be non-decreasing and cover the records of the index, n_tar <= n_assemblies,
 * windowsize >= 1 (SW_ERR_VALUE otherwise).  keep_rows != 0 keeps the table of all rows for sw_markers_export_rows (the
 * reference drops `loc`, markers.py:174-180). */
int sw_index_marker_locs(const sw_index *kept, const sw_subgraphs *sg, const uint32_t *record_offsets, uint64_t n_assemblies,
                         uint64_t n_tar, uint64_t kmerlen, uint64_t windowsize, int keep_rows, sw_markers **out);
/* The same on host arrays (what _get_create_ck_args hands to _create_ck, markers.py:389-425): nodes strictly ascending by hash
 * with [start, stop) into kmers, the occurrences of a node strictly ascending by (record_idx, pos); subgraph s holds the nodes
 * sg_nodes[sg_offsets[s] .. sg_offsets[s + 1]) (indices into nodes). */
int sw_marker_locs_from_arrays(const sw_kmer *kmers, uint64_t n_kmers, const sw_node *nodes, uint64_t n_nodes,
                               const uint64_t *sg_offsets, const uint64_t *sg_nodes, uint64_t n_sg, const uint32_t *record_offsets,
                               uint64_t n_assemblies, uint64_t n_tar, uint64_t kmerlen, uint64_t windowsize, int keep_rows,
                               sw_markers **out);
/* Subgraphs, hashes of all representative orderings, rows, hashes of all rows' orderings (0 unless the rows were kept). */
int sw_markers_sizes(const sw_markers *m, uint64_t *n_sg, uint64_t *n_rep_kmers, uint64_t *n_rows, uint64_t *n_row_kmers);
/* D2H copies (any pointer may be NULL): reps[n_sg], rep_offsets[n_sg + 1] into rep_hashes[n_rep_kmers]. */
int sw_markers_export(const sw_markers *m, sw_marker_rep *reps, uint64_t *rep_offsets, uint64_t *rep_hashes);
/* The rows of subgraph s are rows[row_offsets[s] .. row_offsets[s + 1]); row r's ordering is
 * row_hashes[kmer_offsets[r] .. kmer_offsets[r + 1]).  SW_ERR_VALUE unless the call kept the rows. */
int sw_markers_export_rows(const sw_markers *m, uint64_t *row_offsets, sw_marker_row *rows, uint64_t *kmer_offsets,
                           uint64_t *row_hashes);
/* counters[4] = { non-empty pairs (rows), pairs sorted in the HBM scratch, items of the largest pair, subgraphs voted in the HBM
 * scratch }; ms[4] = { counts + offsets, rows, vote, results } (HIP events). */
int sw_markers_stats(const sw_markers *m, uint64_t *counters, double *ms);
void sw_markers_free(sw_markers *m);

/* ---- markers._fetch_cks_seq (src/seqwin/markers.py:428-471) and row edit distances on the device (csrc/seqs.hip) ---------------
 * An interval is bases [start, stop) of record `record`, the batch's GLOBAL record index (record_offsets[assembly] + the record's
 * index inside its assembly).  start <= stop <= the record's length, record below the batch's records: anything else is
 * SW_ERR_VALUE naming the first such interval. */
typedef struct sw_interval {
    uint32_t record;
    uint32_t start;
    uint32_t stop;
} sw_interval;
#define SW_SEQ_INEXACT 1u /* the interval is not contained in one valid run: it holds a base that was no A, C, G, T (or U) in the file */
typedef struct sw_seqs sw_seqs; /* opaque device-resident text of a list of intervals */
/* Replaces Assemblies.fetch_seq / _fetch_seq (src/seqwin/assemblies.py:101-141, 282-297), which load every FASTA file again
 * (utils.load_fasta, utils.py:492-530: the record text, upper-cased, sliced [start:stop]): the text of the intervals decoded from
 * the resident packed bases -- A, C, G, T and N for every invalid base, as sw_batch_record writes them.  An interval without
 * SW_SEQ_INEXACT is the reference's string (a U of the file reads as T). */
int sw_batch_fetch(const sw_batch *b, const sw_interval *intervals, uint64_t n, sw_seqs **out);
/* The same for the rows of a marker table -- markers._fetch_cks_seq, markers.py:428-471: rows == 0 the representatives, its
 * rep_only; rows != 0 every row, which needs the rows kept -- of subgraphs select[0 .. n_select), in that order -- the intervals are
 * made on the device.  SW_ERR_VALUE unless the batch's record table starts with the one the markers were located with. */
int sw_markers_fetch(const sw_markers *m, const sw_batch *b, int rows, const uint64_t *select, uint64_t n_select, sw_seqs **out);
/* Intervals and bytes of all their text (either may be NULL). */
int sw_seqs_sizes(const sw_seqs *s, uint64_t *n, uint64_t *bytes);
/* D2H copies (any pointer may be NULL): offsets[n + 1] into blob[bytes], flags[n] (SW_SEQ_INEXACT). */
int sw_seqs_export(const sw_seqs *s, uint64_t *offsets, char *blob, uint8_t *flags);
/* counters[2] = { launches of the decode kernel, bytes written }; ms[1] = { checks, offsets and decode } (HIP events). */
int sw_seqs_stats(const sw_seqs *s, uint64_t *counters, double *ms);
void sw_seqs_free(sw_seqs *s);
/* No counterpart in the reference, which judges a candidate through BLAST alone (markers._eval_cks, markers.py:531-722); this is
 * NOT BLAST and fills none of MarkerMetrics.  For n pairs of intervals (r[i], s[i]) of one batch, by DESIGN.md section 3.2c: the
 * symbols are the four valid bases, an invalid base equals nothing (not even another invalid base) and its complement is invalid;
 * d_fwd = the Levenshtein distance of R and S (substitution, insertion, deletion cost 1 each, both consumed whole), d_rev = that of
 * R and the reverse complement of S; dist[i] = min(d_fwd, d_rev), strand[i] = 0 if d_fwd <= d_rev, else 1; a pair with an empty
 * side has the other side's length and strand 0.  Exact for every pair.
 * counters[6] (may be NULL) = { pairs, sum of |R| |S|, pairs done by the striped route (pattern above the block bound), longest
 * side, kernel launches, the block bound }; ms[2] (may be NULL) = { checks + classes, distance kernels } (HIP events). */
int sw_batch_edit_distances(const sw_batch *b, const sw_interval *r, const sw_interval *s, uint64_t n, uint32_t *dist, uint8_t *strand,
                            uint64_t *counters, double *ms);
/* The same with R = the representative of a subgraph and S = each of its rows (what markers._eval_cks, markers.py:531-722, asks
 * BLAST about, answered for the located copies only): one entry per kept row of subgraphs select[0 .. n_select), in that order,
 * the rows of a subgraph ascending by assembly.  Needs the rows kept; record table as for sw_markers_fetch. */
int sw_markers_row_distances(const sw_markers *m, const sw_batch *b, const uint64_t *select, uint64_t n_select, uint32_t *dist,
                             uint8_t *strand, uint64_t *counters, double *ms);

/* ---- Assemblies.mash (src/seqwin/assemblies.py:76-99) on the device (csrc/minhash.hip) ---------------------------------------
 * MinHash sketches as `mash sketch -k K -s S` makes them, one per assembly, and the counts `mash dist` derives for a pair, by the
 * specification of DESIGN.md section 3 (Mash 2.x at its defaults; tests/tools/minhash_host.py restates it -- the `mash` binary
 * itself has never been compared).  Hash: MurmurHash3_x64_128 over the k upper-case ASCII bytes of the canonical k-mer, its first
 * 8 bytes for k >= 17, its first 4 for k <= 16 (a 32-bit sketch).  A sketch: the s smallest distinct hashes of the assembly,
 * ascending.  A pair: the two ascending lists are walked together until s distinct values were seen or a list ran out -- shared =
 * the values met in both, total = the values seen, completed by what is left of either list and clamped to s. */
typedef struct sw_minhash sw_minhash; /* opaque device-resident sketches in CSR form */
/* Replaces `mash sketch` (mash.sketch as Assemblies.mash calls it, assemblies.py:89-96) over a RESIDENT batch: one sketch per
 * assembly.  k outside 1..32 (Mash refuses it too), s = 0 or above 2^32 - 1, seed above 2^32 - 1 (Mash's default: 42), a NULL
 * handle -> SW_ERR_VALUE.  `stream` is a hipStream_t (0 = default stream); the call returns with the sketches finished. */
int sw_batch_minhash(const sw_batch *batch, uint64_t k, uint64_t s, uint64_t seed, void *stream, sw_minhash **out);
/* The sketches given as host arrays (what a .msh file holds): sketch a = hashes[offsets[a] .. offsets[a + 1]), hash_bits 32 or
 * 64.  SW_ERR_VALUE for a list that is not strictly ascending, is longer than s, or -- at 32 bits -- holds a value above
 * 2^32 - 1 (checked on the host, before a device is touched).  The same pair and reduce core then works on them. */
int sw_minhash_from_sketches(const uint64_t *offsets, const uint64_t *hashes, uint64_t n, uint64_t s, uint64_t hash_bits,
                             sw_minhash **out);
/* Sketches, hashes of all sketches, s, hash_bits (any pointer may be NULL). */
int sw_minhash_sizes(const sw_minhash *h, uint64_t *n, uint64_t *n_hashes, uint64_t *s, uint64_t *hash_bits);
/* D2H copies (either may be NULL): offsets[n + 1], hashes[n_hashes] (32-bit sketches widened to uint64). */
int sw_minhash_export(const sw_minhash *h, uint64_t *offsets, uint64_t *hashes);
/* Replaces `mash dist` + the parse of its text (mash.get_jaccard as assemblies.py:97-99 consumes it) for rows [r0, r1) against
 * columns [c0, c1): shared / total of pair (r, c) at [(r - r0) * (c1 - c0) + (c - c0)] of the two host arrays; Jaccard is their
 * quotient.  Two empty sketches give (0, 0).  A range outside the sketches or r0 > r1 -> SW_ERR_VALUE. */
int sw_minhash_counts(const sw_minhash *h, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *shared, uint32_t *total);
/* kmers._expected_frac (src/seqwin/kmers.py:315-323) of the same block, up to the final mean: rowsums[r - r0] = sum over the
 * row's columns of 2J / (1 + J), J = shared / total in f64, added in a fixed order (the same call twice gives the same bits); the
 * caller adds the rows and divides by the number of pairs.  A 0 / 0 pair in the block fails the call: SW_ERR_VALUE, "division by
 * zero" in the message. */
int sw_minhash_frac_rowsums(const sw_minhash *h, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, double *rowsums);
/* counters[4] = { assemblies finished by the general route (all k-mers hashed, sorted, first s distinct), candidates kept by the
 * pre-selection, largest candidate count of an assembly, capacity of an assembly's candidate range }; ms[2] = { hash + pre-select
 * pass, selection with the general route } (HIP events).  All 0 for sketches given as host arrays. */
int sw_minhash_stats(const sw_minhash *h, uint64_t *counters, double *ms);
void sw_minhash_free(sw_minhash *h);

/* ---- exact k-mer containment of query sequences in every assembly (csrc/screen.hip) ---------------------------------------------
 * Stands where markers.eval_markers (src/seqwin/markers.py:607-696) BLASTs every representative against every assembly.  There is
 * no counterpart in the reference: this is NOT BLAST and fills none of MarkerMetrics.  By DESIGN.md section 3.2d
 * (tests/tools/screen_host.py restates it): the alphabet is ACGTU in either case, U reads as T, every other byte is invalid; a
 * k-mer is a window of k valid bases inside one record and one valid run of the batch, or inside one query; its canonical form is
 * the smaller of its 2k-bit word (A0 C1 G2 T3, first base most significant) and its reverse complement's.  counts[q][a] = how many
 * of query q's DISTINCT canonical k-mers occur anywhere in assembly a -- multiplicity never counts, keys are the full words, nothing
 * is hashed into a shorter identity and nothing is approximate. */
typedef struct sw_screen sw_screen; /* opaque: the device-resident counts of one call */
/* Query q is blob[offsets[q] .. offsets[q + 1]); offsets[0] = 0, non-decreasing.  k outside 1..32 (checked before a device is
 * touched), a NULL handle, 2^32 - 256 or more bytes of query text, 2^31 or more distinct query k-mers -> SW_ERR_VALUE.  Zero
 * queries give a 0 x n result.  The batch must be resident.  `stream` is a hipStream_t (0 = default stream); the call returns
 * with the counts finished. */
int sw_batch_screen(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, void *stream,
                    sw_screen **out);
/* Queries, assemblies, distinct canonical k-mers of all queries, k (any pointer may be NULL). */
int sw_screen_sizes(const sw_screen *h, uint64_t *n_queries, uint64_t *n_assemblies, uint64_t *n_distinct, uint64_t *k);
/* n_kmers[n_queries]: the distinct canonical k-mers of every query (0 for a query shorter than k or without a valid window). */
int sw_screen_n_kmers(const sw_screen *h, uint32_t *n_kmers);
/* Rows (queries) [r0, r1) x columns (assemblies) [c0, c1): counts of pair (r, c) at [(r - r0) * (c1 - c0) + (c - c0)] of the host
 * array.  A range outside the result or r0 > r1 -> SW_ERR_VALUE. */
int sw_screen_counts(const sw_screen *h, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *counts);
/* counters[10] = { bytes of query text (query positions), valid query k-mers, distinct query k-mers, slots of the table, most slots
 * a key visited at insertion, batch k-mers probed, hits (multiplicity counted), atomics issued into the bitmap, chunks of
 * assemblies, launches of the probe kernel }; ms[3] = { query side with the table build, probe, reduce } (HIP events; probe and
 * reduce summed over the chunks). */
int sw_screen_stats(const sw_screen *h, uint64_t *counters, double *ms);
/* probe_ms[chunks], reduce_ms[chunks] (either may be NULL): the two times of every chunk of assemblies, in order. */
int sw_screen_chunk_ms(const sw_screen *h, double *probe_ms, double *reduce_ms);
void sw_screen_free(sw_screen *h);

/* ---- k-mer profile: per position of the query text, in how many assemblies of every group the k-mer that starts there occurs
 * ANYWHERE, and how many copies the group holds (csrc/screen.hip; DESIGN.md section 3.2m is the specification,
 * tests/tools/kprofile_host.py restates it).  None of this has a counterpart in the reference; it is NOT BLAST and fills none of
 * MarkerMetrics.  Queries, alphabet, k, windows and canonical words are sw_batch_screen's; the groups are the pileup's: one label per
 * assembly, 0 .. n_groups - 1 with n_groups in 1..8, 255 leaves the assembly out.  Row p of the tables is byte p of the query text
 * (offsets[q] + u).  present[p][g] = the assemblies labelled g that hold the canonical k-mer of the window starting at p in at least
 * one valid window; copies[p][g] = the valid windows of those assemblies whose canonical word equals it (a window counts once,
 * whatever its strand).  A row where no window starts -- the last k - 1 bytes of a query, a window with an invalid byte, a query
 * shorter than k -- reads all ones in both tables, in every group. */
/* (no counterpart in the reference)  sw_batch_screen plus the profile: *out answers everything sw_batch_screen's result answers, bit
 * for bit, and the profile getters below.  copies != 0 also counts the copies.  n_groups outside 1..8 or a label in
 * n_groups .. 254 -> SW_ERR_VALUE before a device is touched.  A single-device call on a resident batch. */
int sw_batch_screen_profile(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k,
                            const uint8_t *labels, uint64_t n_groups, int copies, void *stream, sw_screen **out);
/* (no counterpart in the reference)  Rows (the bytes of the query text), groups, whether copies were counted (any pointer may be
 * NULL).  This and the three getters below: SW_ERR_VALUE for a screen made by sw_batch_screen. */
int sw_screen_profile_sizes(const sw_screen *h, uint64_t *rows, uint64_t *n_groups, uint64_t *has_copies);
/* (no counterpart in the reference)  D2H copy: present[rows * n_groups], copies[rows * n_groups] (NULL: not wanted; SW_ERR_VALUE
 * if they were not counted), group_sizes[n_groups] = the assemblies of every label (any pointer may be NULL). */
int sw_screen_profile_export(const sw_screen *h, uint32_t *present, uint64_t *copies, uint32_t *group_sizes);
/* (no counterpart in the reference)  counters[2] = { bytes of the profile's device tables (per k-mer, per position and the map
 * between them), copy adds issued by the probe }; ms[2] = { the transposed reduction k_scr_profile summed over the chunks, the
 * gather } (HIP events).  With a profile, sw_screen_stats' reduce time does not contain the transposed reduction. */
int sw_screen_profile_stats(const sw_screen *h, uint64_t *counters, double *ms);

/* ---- the best hit of every query in every assembly: seed vote + infix edit distance (csrc/hits.hip) ------------------------------
 * Covers the ground of markers.eval_markers' output (src/seqwin/markers.py:531-604 keeps the best BLAST hit's nident, mismatch and
 * gaps per (query, assembly)) with an exactly specified quantity of its own.  There is no counterpart in the reference: this is NOT
 * BLAST, has no scores, no e-values and no local alignment, and fills none of MarkerMetrics.  DESIGN.md section 3.2e is the
 * specification, tests/tools/hits_host.py restates it.  Queries, alphabet, k-mers and canonical words are those of the screen. */
typedef struct sw_infix_pair {
    uint32_t query;  /* index into the queries of the call */
    uint32_t strand; /* 0: the query; 1: its reverse complement */
    uint32_t record; /* the batch's global record index */
    uint32_t start;
    uint32_t stop;   /* the text: bases [start, stop) of the record */
} sw_infix_pair;
/* Layer A.  For n pairs: the pattern P is the query (strand 0) or its reverse complement (strand 1), the text T the interval; an
 * invalid base equals nothing and its complement is invalid (section 3.2c).  With D[0][j] = 0, D[i][0] = i and the unit-cost
 * Levenshtein recurrence: dist[i] = min over 0 <= j <= |T| of D[|P|][j] (the text's ends are free, the pattern is consumed whole),
 * end[i] = start + the smallest j that attains it.  An empty query gives (0, start), an empty text (|P|, start).  Exact for every
 * pair.  A pair that names no query, a strand above 1 or start > stop (checked before a handle or a device is touched), or an
 * interval outside its record -> SW_ERR_VALUE.  counters[6] (may be NULL) = { pairs, sum of |P| |T|, pairs done by the striped
 * route (query above the block bound), longest query, kernel launches, the block bound }; ms[1] (may be NULL) = { classes and
 * distance kernels } (HIP events). */
int sw_batch_infix_distances(const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs,
                             uint64_t n, uint32_t *dist, uint32_t *end, uint64_t *counters, double *ms);
typedef struct sw_hits sw_hits; /* opaque: the device-resident [n_queries][n_assemblies] results of one call */
/* Layer B.  A canonical word is a seed iff exactly one valid window of ALL query text has it (both orientations are one word) and it
 * is not its own reverse complement; every window of the batch whose canonical word is a seed is a hit (record r, position p,
 * orientation o); hits vote for bands of 64 implied end positions, the winner of a (query, assembly) is the (r, o, b) with the
 * largest c[b] + c[b + 1], ties to the smallest (r, o, b); Layer A on the winner's window gives dist and end.  A pair without a hit
 * reads seeds = 0, record = end = dist = 0xFFFFFFFF, strand = 0.  k outside 1..32 (checked before a device is touched), a NULL
 * handle, key fields that do not fit 64 bits -> SW_ERR_VALUE.  The batch must be resident; the call works on the default stream of
 * the batch's device and returns with the results finished. */
int sw_batch_best_hits(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, sw_hits **out);
/* Queries, assemblies, seeds of all queries, k (any pointer may be NULL). */
int sw_hits_sizes(const sw_hits *h, uint64_t *n_queries, uint64_t *n_assemblies, uint64_t *n_seeds, uint64_t *k);
/* n_seeds[n_queries]: the seeds of every query. */
int sw_hits_n_seeds(const sw_hits *h, uint32_t *n_seeds);
/* Rows (queries) [r0, r1) x columns (assemblies) [c0, c1) of one field -- 0 seeds, 1 record, 2 strand, 3 end, 4 dist --: pair (r, c)
 * at [(r - r0) * (c1 - c0) + (c - c0)] of the host array.  A range outside the result, r0 > r1 or another field -> SW_ERR_VALUE. */
int sw_hits_block(const sw_hits *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out);
/* counters[10] = { hits, seeds, chunks of assemblies, chunk splits, launches of the probe kernel, pairs aligned, pairs on the striped
 * route, distinct query k-mers, keys the hit buffer held at the end, doublings of the buffer }; ms[4] = { query side, probe, sort +
 * vote, distances } (HIP events, summed over the chunks). */
int sw_hits_stats(const sw_hits *h, uint64_t *counters, double *ms);
/* hits[chunks]: the hits of every chunk of assemblies, in order. */
int sw_hits_chunk_hits(const sw_hits *h, uint64_t *hits);
void sw_hits_free(sw_hits *h);

/* ---- the alignment behind a best hit: start, nident, mismatch, gaps, edit script (csrc/align.hip) ---------------------------------
 * The canonical optimal alignment of Layer A's pair, by DESIGN.md section 3.2f (tests/tools/align_host.py restates it).  Still NOT
 * BLAST: no scores, no e-values, no local alignment, none of MarkerMetrics.  With D the infix matrix of Layer A and (m, j*) the cell
 * that gave dist and end, the traceback repeats, first match wins, until i = 0: (1) j > 0 and P[i-1] = T[j-1], both valid: `=`, to
 * (i-1, j-1); (2) j > 0 and D[i-1][j-1] + 1 = D[i][j]: `X`, to (i-1, j-1); (3) D[i-1][j] + 1 = D[i][j]: `I`, a pattern base faces a
 * gap, to (i-1, j); (4) otherwise `D`, a text base faces a gap, to (i, j-1).  a_start = start + j at the stop, nident = #`=`,
 * mismatch = #`X`, gaps = #`I` + #`D`: nident + mismatch + #I = |P|, nident + mismatch + #D = end - a_start, mismatch + gaps =
 * dist.  An empty query gives a_start = end = start and no ops, an empty text a_start = start and |P| ops `I`. */
typedef struct sw_ops sw_ops; /* opaque: the edit scripts of one sw_batch_infix_alignments call, CSR, on the device */
/* sw_batch_infix_distances plus the traceback of every pair: the same arguments, checks and errors; a_start, nident, mismatch and
 * gaps are host arrays of n like dist and end.  ops != NULL: *ops receives the scripts -- pair i's ops in pattern order from a_start
 * to end, one byte each (0 `=`, 1 `X`, 2 `I`, 3 `D`), |P| + #D of them.  counters[8] (may be NULL) = { pairs traced, rounds through
 * the scratch, pairs on the striped route, pairs with a scratch of their own, scratch bytes at peak, ops written, largest scratch of
 * one pair in bytes, launches of the store kernels }; ms[3] (may be NULL) = { distances, store pass, walk } (HIP events). */
int sw_batch_infix_alignments(const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs,
                              uint64_t n, uint32_t *dist, uint32_t *end, uint32_t *a_start, uint32_t *nident, uint32_t *mismatch, uint32_t *gaps,
                              sw_ops **ops, uint64_t *counters, double *ms);
/* Pairs and bytes of all their scripts (either may be NULL). */
int sw_ops_sizes(const sw_ops *o, uint64_t *n, uint64_t *bytes);
/* D2H copies (either may be NULL): offsets[n + 1] into ops[bytes]. */
int sw_ops_export(const sw_ops *o, uint64_t *offsets, uint8_t *ops);
void sw_ops_free(sw_ops *o);
/* sw_batch_best_hits plus the traceback of every winner, run once per chunk of assemblies right behind the chunk's distances.  The
 * five fields of sw_hits_block are what sw_batch_best_hits gives. */
int sw_batch_best_hits_aligned(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, sw_hits **out);
/* sw_hits_block for the fields 0 a_start, 1 nident, 2 mismatch, 3 gaps; a pair without a hit reads 0xFFFFFFFF in all four.  Hits made
 * by sw_batch_best_hits hold none of them: SW_ERR_VALUE. */
int sw_hits_align_block(const sw_hits *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out);
/* counters[8] as for sw_batch_infix_alignments, summed over the chunks (the two peaks: the largest); ms[2] = { store pass, walk }.
 * SW_ERR_VALUE for hits made without the alignment. */
int sw_hits_align_stats(const sw_hits *h, uint64_t *counters, double *ms);

/* ---- every seeded locus of a (query, assembly) pair: repeat counts and the sum of nident (csrc/hits.hip, loci mode) -----------------
 * Stands where eval_markers' n_hits / avg_nident columns stand; by DESIGN.md section 3.2g (tests/tools/loci_host.py restates it).
 * Still NOT BLAST and fills none of MarkerMetrics.  A candidate (r, o, b) of section 3.2e is a locus iff its score reaches min_seeds
 * and no candidate of the same (query, r, o) within two bands has a larger score, or the same score in a smaller band.  Every locus
 * gets the window, the distance and the canonical alignment a winner gets.  The list ascends by (query, record, orientation, band);
 * locus j is a duplicate iff locus j - 1 has the same query, record, strand, a_start and end.  Per (query, assembly): n_loci counts
 * the loci that are no duplicates, sum_nident adds their nident; 0 where there is none.
 * sw_batch_best_hits_aligned plus the loci: the fields of sw_hits_block / sw_hits_align_block are what that call gives, whatever
 * min_seeds is.  min_seeds == 0 (checked before a device is touched, behind k), the largest n_loci times the longest query reaching
 * 2^32 -> SW_ERR_VALUE. */
int sw_batch_best_hits_loci(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, uint64_t min_seeds,
                            sw_hits **out);
/* Loci of all pairs, and how many of them are duplicates (either may be NULL).  This and the three calls below: SW_ERR_VALUE for hits
 * made without the loci. */
int sw_hits_loci_sizes(const sw_hits *h, uint64_t *n_loci_total, uint64_t *n_dup);
/* D2H copies, a NULL array is skipped: cell_offsets[n_queries * n_assemblies + 1] -- the loci of pair (q, a) are entries
 * [cell_offsets[q * n_assemblies + a], cell_offsets[q * n_assemblies + a + 1]) --, and the list's columns, n_loci_total entries each
 * (strand and dup are 0 or 1). */
int sw_hits_loci(const sw_hits *h, uint64_t *cell_offsets, uint32_t *query, uint32_t *assembly, uint32_t *record, uint32_t *strand, uint32_t *band,
                 uint32_t *seeds, uint32_t *dist, uint32_t *end, uint32_t *a_start, uint32_t *nident, uint32_t *mismatch, uint32_t *gaps, uint32_t *dup);
/* sw_hits_block for the fields 0 n_loci, 1 sum_nident. */
int sw_hits_loci_block(const sw_hits *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out);
/* counters[5] = { loci, duplicates, most loci of one pair (duplicates not counted), pairs aligned for the list, rounds of their
 * traceback through the scratch }; ms[4] = { peaks + compaction, distances, traceback, final ordering + reduction } (HIP events,
 * the first three summed over the chunks). */
int sw_hits_loci_stats(const sw_hits *h, uint64_t *counters, double *ms);

/* ---- seeds shared between queries, up to a cap of copies (csrc/hits.hip, k_hit_probe_shared) --------------------------------------
 * By DESIGN.md section 3.2h (tests/tools/shared_seeds_host.py restates it).  mult(word) = the valid windows of ALL query text whose
 * canonical word it is.  With seed_copies = c: a word is a seed iff 1 <= mult <= c and it is not its own reverse complement, and
 * every one of its windows (query, offset, window-is-canonical) owns it; a word with mult > c is dropped whole.  n_seeds[q] counts
 * the windows of q that own a seed.  A window of the batch whose word is a seed is one hit per owner, each by Layer B's formulas with
 * that owner's query, offset and orientation; from the hits on -- vote, ties, winners, windows, distances, alignments, loci --
 * everything is Layer B's.  At c = 1 every output equals the corresponding call above bit for bit.
 * mode: 0 as sw_batch_best_hits, 1 as sw_batch_best_hits_aligned, 2 as sw_batch_best_hits_loci; min_seeds is read in mode 2 only.
 * The result answers every sw_hits_* call its mode's call answers.  seed_copies outside 1..256, a mode above 2, min_seeds == 0 in
 * mode 2 (all checked before a device is touched), more than 2^31 queries -> SW_ERR_VALUE; the rest as sw_batch_best_hits. */
int sw_batch_best_hits_shared(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, uint64_t seed_copies,
                              uint64_t mode, uint64_t min_seeds, sw_hits **out);
/* counters[8] = { seed_copies (0: made by one of the calls above, whose rule is the one at c = 1), seed words kept, windows that own
 * them, words dropped for mult > c, the windows dropped with them, words that are their own reverse complement (whatever their
 * mult; they are not counted as dropped), the longest owner list, hits appended over all chunks }. */
int sw_hits_seed_stats(const sw_hits *h, uint64_t *counters);

/* ---- local alignments with affine gap scores at every pair of Layer A (csrc/local.hip) ---------------------------------------------
 * By DESIGN.md section 3.2i (tests/tools/local_host.py restates it twice).  It is NOT BLAST: the seeds and the window are ours, the
 * dynamic programme is exhaustive inside the window (no X-drop), there is no e-value filter, no bit score, and none of
 * MarkerMetrics is filled.  A pair is Layer A's: pattern P = the query or its reverse complement (m bases), text T = [start, stop)
 * of the record (n bases); an invalid base equals nothing.  Scoring (reward r in 1..255, penalty p in -255..-1, gapopen go in
 * 0..255, gapextend ge in 1..255; blastn's defaults are 2, -3, 5, 2): a gap of L columns costs go + L * ge.
 *   E[i][j] = max(E[i][j-1], H[i][j-1] - go) - ge      F[i][j] = max(F[i-1][j], H[i-1][j] - go) - ge
 *   H[i][j] = max(0, H[i-1][j-1] + s(i,j), E[i][j], F[i][j]),  borders H = 0, E = F = -infinity
 * Every value carries the record (i0, j0, mismatch, gapopen, gaps) of one canonical alignment: H = 0 carries (i, j, 0, 0, 0);
 * extension wins a tie against opening; a positive H takes the first of diagonal, E, F that attains the maximum.  score = max H at
 * the maximal cell (i*, j*) with the smallest j, then the smallest i; qstart = i0, qend = i* (half-open, in P's orientation),
 * sstart = start + j0, send = start + j*; ins = (gaps + (i* - i0) - (j* - j0)) / 2, nident = (i* - i0) - mismatch - ins.
 * score == 0 (an empty side, or no match): every count 0, qstart = qend = 0, sstart = send = start. */
typedef struct sw_scoring {
    int32_t reward, penalty, gapopen, gapextend;
} sw_scoring;
/* The nine figures of n pairs (host arrays of n; any of them may be NULL).  Checks and errors are sw_batch_infix_distances';
 * a scoring value outside its range, a NULL scoring, or a pair with m >= 2^16 or n >= 2^16 -> SW_ERR_VALUE, all before a device is
 * touched.  counters[6] (or NULL) = { pairs, sum of m * n, pairs in more than one stripe, pairs with an HBM carry row, launches, rows
 * of a group pass }; ms[1] (or NULL): the kernels (HIP events). */
int sw_batch_local_alignments(const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs,
                              uint64_t n, const sw_scoring *scoring, uint32_t *score, uint32_t *qstart, uint32_t *qend, uint32_t *sstart,
                              uint32_t *send, uint32_t *nident, uint32_t *mismatch, uint32_t *gapopen, uint32_t *gaps, uint64_t *counters,
                              double *ms);
/* Best hits with the local alignment of every winner (and, in mode 2, of every locus) on its window.  seed_copies 0: the
 * unique-seed route, else as sw_batch_best_hits_shared; mode and min_seeds as there.  Everything that mode's call returns is
 * returned bit for bit; in addition nine [n_queries][n_assemblies] fields (sw_hits_local_block; a cell without a hit holds
 * 0xFFFFFFFF) and, in mode 2, nine list columns in the loci's order (sw_hits_loci_local).  A query above 65279 bases (its window
 * would reach 2^16) or a scoring value outside its range -> SW_ERR_VALUE before a device is touched. */
int sw_batch_best_hits_local(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, uint64_t seed_copies,
                             uint64_t mode, uint64_t min_seeds, const sw_scoring *scoring, sw_hits **out);
/* field: 0 score, 1 qstart, 2 qend, 3 sstart, 4 send, 5 nident, 6 mismatch, 7 gapopen, 8 gaps.  These three return SW_ERR_VALUE for
 * hits made without the local alignment (sw_hits_loci_local also for hits made without the loci). */
int sw_hits_local_block(const sw_hits *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out);
int sw_hits_loci_local(const sw_hits *h, uint32_t *score, uint32_t *qstart, uint32_t *qend, uint32_t *sstart, uint32_t *send, uint32_t *nident,
                       uint32_t *mismatch, uint32_t *gapopen, uint32_t *gaps);
/* counters[6] and ms[1] as sw_batch_local_alignments', summed over the chunks, winners and loci together. */
int sw_hits_local_stats(const sw_hits *h, uint64_t *counters, double *ms);

/* ---- pileup: base counts per query position over the canonical alignments, by group (csrc/align.hip, the pile walk) ---------------
 * By DESIGN.md section 3.2k (tests/tools/pileup_host.py restates it twice).  It is NOT BLAST and no multiple alignment: every pair
 * is aligned to its query alone, and none of MarkerMetrics is filled.  The table is uint32 T[total query bases][n_groups][8], the
 * queries one behind the other as in the call's CSR; the classes are A 0, C 1, G 2, T 3, N 4, DEL 5, INS 6, INS_BASES 7.  Walking a
 * pair's script (section 3.2f) with pattern index i' and m = |query|: `=` / `X` add 1 to the class of the text base they face (an
 * invalid one: N) at query position u = i' (strand 0) or m - 1 - i' with the base complemented (strand 1); `I` adds 1 to DEL at the
 * same u; a maximal run of L `D` before pattern index i' adds 1 to INS and L to INS_BASES at u = i' (strand 0) or m - i' (strand 1),
 * always 1 <= u <= m - 1.  depth[q][g] counts the pairs of query q piled into group g; A + C + G + T + N + DEL = depth at every
 * position.  A pair is piled iff its label is below n_groups and dist * 1000 <= max_dist_permille * m; label 255 leaves it out.
 * n_groups outside 1..8, max_dist_permille above 1000, a label in n_groups..254, (pairs of the call or assemblies of the batch)
 * times the longest query reaching 2^32 -> SW_ERR_VALUE before a device is touched.  Nothing depends on the order of the pairs. */
typedef struct sw_pileup sw_pileup; /* opaque: the device-resident table and depths of one call */
/* sw_batch_infix_alignments without scripts -- the same six arrays, checks and errors, counters[8] and ms[3] -- whose walk also piles
 * pair i into group pair_group[i]. */
int sw_batch_infix_pileup(const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs, uint64_t n,
                          const uint8_t *pair_group, uint64_t n_groups, uint64_t max_dist_permille, uint32_t *dist, uint32_t *end, uint32_t *a_start,
                          uint32_t *nident, uint32_t *mismatch, uint32_t *gaps, sw_pileup **out, uint64_t *counters, double *ms);
/* Best hits whose winners are piled, the winner of assembly a into group assembly_group[a].  seed_copies 0: the unique-seed route,
 * else as sw_batch_best_hits_shared; mode 0 is treated as 1 (the pile needs the alignment), 2 adds the loci, which are not piled;
 * scoring may be NULL, else as sw_batch_best_hits_local.  Everything *out answers is bit for bit what the same call without the pile
 * answers. */
int sw_batch_best_hits_pileup(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, uint64_t seed_copies,
                              uint64_t mode, uint64_t min_seeds, const sw_scoring *scoring, const uint8_t *assembly_group, uint64_t n_groups,
                              uint64_t max_dist_permille, sw_hits **out, sw_pileup **pile);
/* Queries, bases of all queries (the table's rows), groups (any pointer may be NULL). */
int sw_pileup_sizes(const sw_pileup *p, uint64_t *n_queries, uint64_t *total_bases, uint64_t *n_groups);
/* D2H copy of the rows of queries [q0, q1): out[(bases of those queries) * n_groups * 8].  A range outside the queries -> SW_ERR_VALUE. */
int sw_pileup_export(const sw_pileup *p, uint64_t q0, uint64_t q1, uint32_t *out);
/* depth[n_queries * n_groups]. */
int sw_pileup_depth(const sw_pileup *p, uint32_t *depth);
/* counters[5] = { pairs piled, pairs filtered by distance, pairs left out by label, adds issued to the table, table bytes };
 * ms[1] = { the pile walk } (HIP events, summed over rounds and chunks).  Either may be NULL. */
int sw_pileup_stats(const sw_pileup *p, uint64_t *counters, double *ms);
void sw_pileup_free(sw_pileup *p);

/* ---- oligo windows: joint mismatch classes per query window over the canonical alignments, by group (csrc/align.hip, the window walk)
 * By DESIGN.md section 3.2l (tests/tools/windows_host.py restates it twice).  It is NOT BLAST and no thermodynamic model (no Tm, no
 * dG), and none of MarkerMetrics is filled.  The table is uint32 W[total query bases][n_lengths][n_groups][8], the queries one behind
 * the other as in the pileup's table, the row the window's start u in query coordinates; rows with u > m - L stay 0.  The pairs that
 * count are the pairs the pileup of section 3.2k piles.  Of a piled pair's script (section 3.2f): x[i'] / ins[i'] say that the column
 * consuming pattern index i' is `X` / `I`, b[i'] (1 <= i' <= m - 1) that a run of `D` lies before i'.  The pattern window [s, s + L)
 * has e = the sum of x over it and is gapped iff an ins lies in it or a b[i'] with s < i' < s + L; it is the query window at
 * u = s (strand 0) or m - L - s (strand 1); right_bad / left_bad: an `X` faces one of its last / first three_prime query positions.
 * The pair adds 1 to exactly one of MM0 0, MM1 1, MM2 2, MM3 3 (ungapped, e = 0..3), MM4P 4 (ungapped, e >= 4), GAPPED 5, and to
 * FWD_OK 6 (ungapped, e <= max_mismatch, not right_bad) and REV_OK 7 (the same with left_bad) where they hold: classes 0..5 add up to
 * the pileup's depth at every u <= m - L.  1..8 distinct lengths, each in 8..32, in the order given; max_mismatch in 0..8 and below
 * the shortest length; three_prime in 0..8; anything else -> SW_ERR_VALUE before a device is touched.  Nothing depends on the order
 * of the pairs. */
typedef struct sw_windows sw_windows; /* opaque: the device-resident window table of one call */
/* sw_batch_infix_pileup -- the same arrays, pileup, checks and errors, counters[8] and ms[3] -- whose walk also classes every window of
 * the n_lengths lengths (section 3.2l).  One walk fills both tables, so the only thing of the pileup that differs from the call
 * without windows is a time: sw_pileup_stats' ms[0] (and ms[2] here) is that one walk's, the figure sw_windows_stats gives too. */
int sw_batch_infix_windows(const sw_batch *b, const uint64_t *offsets, const char *blob, uint64_t n_queries, const sw_infix_pair *pairs, uint64_t n,
                           const uint8_t *pair_group, uint64_t n_groups, uint64_t max_dist_permille, const uint32_t *lengths, uint64_t n_lengths,
                           uint64_t max_mismatch, uint64_t three_prime, uint32_t *dist, uint32_t *end, uint32_t *a_start, uint32_t *nident,
                           uint32_t *mismatch, uint32_t *gaps, sw_pileup **out, sw_windows **windows, uint64_t *counters, double *ms);
/* sw_batch_best_hits_pileup whose winners' walk also classes every window (section 3.2l).  Everything *out and *pile answer is bit for
 * bit what the same call without the windows answers, but for the times: the pile walk's is that of the one walk that fills both. */
int sw_batch_best_hits_windows(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_queries, uint64_t k, uint64_t seed_copies,
                               uint64_t mode, uint64_t min_seeds, const sw_scoring *scoring, const uint8_t *assembly_group, uint64_t n_groups,
                               uint64_t max_dist_permille, const uint32_t *lengths, uint64_t n_lengths, uint64_t max_mismatch, uint64_t three_prime,
                               sw_hits **out, sw_pileup **pile, sw_windows **windows);
/* Section 3.2l: queries, bases of all queries (the table's rows), groups, lengths, max_mismatch, three_prime (any pointer may be NULL). */
int sw_windows_sizes(const sw_windows *w, uint64_t *n_queries, uint64_t *total_bases, uint64_t *n_groups, uint64_t *n_lengths, uint64_t *max_mismatch,
                     uint64_t *three_prime);
/* Section 3.2l: lengths[n_lengths], in the order the call gave them. */
int sw_windows_lengths(const sw_windows *w, uint32_t *lengths);
/* Section 3.2l: D2H copy of the rows of queries [q0, q1): out[(bases of those queries) * n_lengths * n_groups * 8].  A range outside
 * the queries -> SW_ERR_VALUE. */
int sw_windows_export(const sw_windows *w, uint64_t q0, uint64_t q1, uint32_t *out);
/* Section 3.2l: counters[3] = { windows visited (of piled pairs, all lengths), adds issued to the table by the walk, table bytes };
 * ms[2] = { the window walk, the finishing kernel } (HIP events, summed over rounds and chunks).  Either may be NULL. */
int sw_windows_stats(const sw_windows *w, uint64_t *counters, double *ms);
/* Section 3.2l. */
void sw_windows_free(sw_windows *w);

/* ---- oligo search: every place where a primer or probe binds with at most d mismatches, on either strand (csrc/oligo.hip) ----
 * None of this has a counterpart in the reference.  It is NOT BLAST (no e-values) and a site is not defined by a thermodynamic
 * model (that is an addition behind the hit: sw_batch_oligo_hits_thermo below); one exactly specified quantity, Hamming distance under IUPAC sets, over EVERY window of the resident batch -- no seed is needed, so no
 * site is missed.  DESIGN.md section 3.2j is the specification, tests/tools/oligo_host.py restates it.
 * An oligo is 8..32 letters in either case: A C G T, U (= T) or an IUPAC code R Y S W K M B D H V N; every position is a set of
 * bases.  P0 is the oligo, P1 its reverse complement (the sets complemented, the order reversed).  A site (oligo, strand s, record,
 * pos) is a window [pos, pos + L) inside one valid run of the record; mm = the number of i with text[pos + i] not in Ps[i].  A hit is
 * a site with mm <= max_mismatch and no mismatch among the three_prime bases at the oligo's 3' end (strand 0: positions L - c ..
 * L - 1 of the window, strand 1: positions 0 .. c - 1).  An oligo that equals its reverse complement hits twice at one place. */
typedef struct sw_oligos sw_oligos; /* opaque: the device-resident [n_oligos][n_assemblies] results of one call, and the site list */
/* (no counterpart in the reference)  Oligos as the queries of sw_batch_screen (CSR over `blob`).  1..4096 oligos of 8..32 IUPAC
 * letters, max_mismatch in 0..8 and below the shortest oligo, three_prime in 0..8: anything else -> SW_ERR_VALUE before a device is
 * touched.  want_sites != 0 also keeps the list of all hits.  A batch of 2^43 bases or more, or a list of 2^32 entries or more ->
 * SW_ERR_RUNTIME.  A single-device call on a resident batch; returns with the results finished. */
int sw_batch_oligo_hits(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_oligos, uint64_t max_mismatch,
                        uint64_t three_prime, int want_sites, void *stream, sw_oligos **out);
/* (no counterpart in the reference)  Oligos, assemblies, max_mismatch, three_prime of the call (any pointer may be NULL). */
int sw_oligos_sizes(const sw_oligos *h, uint64_t *n_oligos, uint64_t *n_assemblies, uint64_t *max_mismatch, uint64_t *three_prime);
/* (no counterpart in the reference)  sw_screen_counts for one field: 0 n_sites (hits on both strands), and of the hit that is least
 * in the order (mm, record, pos, strand): 1 best_mm, 2 best_record (global), 3 best_pos, 4 best_strand -- 0xFFFFFFFF without a hit. */
int sw_oligos_block(const sw_oligos *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out);
/* (no counterpart in the reference)  Entries of the site list.  This and sw_oligos_sites: SW_ERR_VALUE for a result made without it. */
int sw_oligos_sites_size(const sw_oligos *h, uint64_t *n_sites_total);
/* (no counterpart in the reference)  Every hit, ascending by (oligo, assembly, record, pos, strand): cell_offsets[n_oligos *
 * n_assemblies + 1] -- the hits of pair (q, a) are the entries [cell_offsets[q * n_assemblies + a], cell_offsets[q * n_assemblies +
 * a + 1]) -- and the list's columns, n_sites_total entries each (record is global, strand 0 or 1). */
int sw_oligos_sites(const sw_oligos *h, uint64_t *cell_offsets, uint32_t *oligo, uint32_t *assembly, uint32_t *record, uint32_t *pos,
                    uint32_t *strand, uint32_t *mm);
/* (no counterpart in the reference)  counters[8] = { windows scanned (window ends of the runs of shortest-oligo length or more, summed
 * over the passes), passes over the batch (groups of oligos), chunks of assemblies, launches of the scan kernel, hits, doublings of
 * the site buffer, chunks redone in halves, window x pattern comparisons (a pattern = an oligo on a strand) }; ms[2] = { scan, order
 * of the site list } (HIP events). */
int sw_oligos_stats(const sw_oligos *h, uint64_t *counters, double *ms);
/* ---- oligo search with indels (csrc/oligo.hip; tests/tools/oligo_edit_host.py restates it) ----
 * The same object by unit-cost edit distance.  On a valid run T of n bases and strand 0, with Q the oligo without its last
 * three_prime = c letters: E(e) = the least ed(Q, T[b : e - c]) over b if the c bases before the end e face the clamp's sets, else
 * infinite; D(e) = min(E(e), d + 1).  The end e is a site iff D(e) <= d, D > D(e) on the d ends before it and D >= D(e) on the d ends
 * after it, inside the run.  Its alignment is the canonical traceback of section 3.2f (rules =, X, I, D in that order) from
 * (|Q|, e - c) until the oligo is used up: pos where it stops, mismatch = #X, gaps = #I + #D, dist = mismatch + gaps = D(e).  Strand 1 is
 * strand 0 on the run's reverse complement, the interval mapped back.  Per cell the best site is the least in (dist, record, pos,
 * strand), then end.  The list is ordered by (oligo, assembly, record, pos, end, strand). */
/* (no counterpart in the reference)  As sw_batch_oligo_hits.  max_edits in 0..4, three_prime in 0..8, max_edits + three_prime below
 * the shortest oligo: anything else -> SW_ERR_VALUE before a device is touched.  max_edits = 0 gives the sites of max_mismatch = 0. */
int sw_batch_oligo_hits_edit(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_oligos, uint64_t max_edits,
                             uint64_t three_prime, int want_sites, void *stream, sw_oligos **out);
/* (no counterpart in the reference)  max_edits of the call; -1 for a result of sw_batch_oligo_hits.  On a result with max_edits
 * sw_oligos_block's field 1 and sw_oligos_sites' mm hold dist, and sw_oligos_block has the fields 5 best_end, 6 best_mismatch and
 * 7 best_gaps; on a Hamming result these three answer pos + L, mm and 0. */
int sw_oligos_max_edits(const sw_oligos *h, int64_t *max_edits);
/* (no counterpart in the reference)  sw_oligos_sites with the columns end, mismatch and gaps in place of mm (dist is their sum); a
 * Hamming result answers pos + L, mm and 0. */
int sw_oligos_sites_edit(const sw_oligos *h, uint64_t *cell_offsets, uint32_t *oligo, uint32_t *assembly, uint32_t *record, uint32_t *pos,
                         uint32_t *strand, uint32_t *end, uint32_t *mismatch, uint32_t *gaps);
/* (no counterpart in the reference)  counters[2] = { steps of the bit-vector column (an upper bound: every lane with an end counts
 * L + 3 max_edits - 1 steps more than it has ends, per oligo and strand), candidates resolved }; ms[1] = { the resolve kernel };
 * zeros for a Hamming result.  With max_edits sw_oligos_stats' scan time excludes the resolve kernel. */
int sw_oligos_edit_stats(const sw_oligos *h, uint64_t *counters, double *ms);
/* ---- oligo search with a nearest-neighbour model (csrc/oligo.hip; tests/tools/oligo_thermo_host.py restates
 * it) ----
 * The hits of sw_batch_oligo_hits, and per hit the sums of the CALLER'S integer tables.  Base codes A=0 C=1 G=2 T=3.  stack is
 * int16[3][4][4][4][4], planes dh (100 cal/mol), ds (0.1 cal/(K mol)), dg (cal/mol), index [x1][x2][y1][y2]: x1 x2 two consecutive
 * oligo bases 5'->3', y1 y2 the bases of the bound strand that face them (y1 pairs with x1).  end is int16[3][2][4][4]: the terminal
 * pair [x][y] at the oligo's 5' end (0) and 3' end (1).  init is int32[3].  For a hit with window text t_0..t_{L-1}: strand 0
 * y_i = 3 - t_{i-1}, strand 1 y_i = t_{L-i}; x_i = 3 - y_i where the oligo's set at i holds it, else the set's least member;
 * (dh, ds, dg) = init + end[0][x_1][y_1] + end[1][x_L][y_L] + the sum of stack[x_i][x_i+1][y_i][y_i+1], in int32.  Per cell: n_stable,
 * the hits with dg <= max_dg, and the MOST STABLE hit, least in (dg, record, pos, strand) among all hits.  Nothing is multiplied by
 * a temperature and no Tm is formed on the device; bulges (max_edits), dimers, hairpins, dangling ends and salt are out of scope. */
/* (no counterpart in the reference)  As sw_batch_oligo_hits, with the model.  Every dg entry and init[2] must satisfy |v| <= 15000
 * (the most stable site's key relies on it): SW_ERR_VALUE otherwise, before a device is touched.  no_threshold != 0: every hit counts
 * as stable and max_dg is ignored. */
int sw_batch_oligo_hits_thermo(const sw_batch *batch, const uint64_t *offsets, const char *blob, uint64_t n_oligos, uint64_t max_mismatch,
                               uint64_t three_prime, int want_sites, void *stream, const int16_t *stack, const int16_t *end,
                               const int32_t *init, int64_t max_dg, int no_threshold, sw_oligos **out);
/* (no counterpart in the reference)  sw_oligos_block for the model's fields, 4 bytes an entry: 0 n_stable (uint32); of the most
 * stable hit 1 stable_dg, 2 stable_dh, 3 stable_ds (int32; INT32_MIN without a hit), 4 stable_record, 5 stable_pos, 6 stable_strand,
 * 7 stable_mm (uint32; 0xFFFFFFFF without a hit).  This and the two below: SW_ERR_VALUE for a result made without a model. */
int sw_oligos_thermo_block(const sw_oligos *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, void *out);
/* (no counterpart in the reference)  dh, ds, dg of every entry of the site list, parallel to sw_oligos_sites' columns. */
int sw_oligos_sites_thermo(const sw_oligos *h, int32_t *dh, int32_t *ds, int32_t *dg);
/* (no counterpart in the reference)  *stable_hits = the sum of n_stable; ms[2] = { the kernel of the most stable sites' fields, the
 * kernel of the list's sums } (HIP events).  sw_oligos_stats' scan time excludes the first. */
int sw_oligos_thermo_stats(const sw_oligos *h, uint64_t *stable_hits, double *ms);
/* (no counterpart in the reference) */
void sw_oligos_free(sw_oligos *h);

/* ---- amplicons: the products of primer pairs, and the probes inside them, over a site list (csrc/amplicons.hip, DESIGN.md section
 * 3.2p; tests/tools/amplicons_host.py restates it) ----
 * None of this has a counterpart in the reference, and it is no in-silico PCR tool.  Exact, in integers, on the site list of a
 * sw_oligos made with want_sites.  A site is (oligo, assembly, record, pos, end, strand, d): on a Hamming result end = pos + L and
 * d = mm, on a result with max_edits the site's own end and dist.  For pair i = (f, r): orientation + (0) joins a site of f on strand
 * 0 at pf with a site of r on strand 1 of the same record with pos_r >= pf, the product is [pf, end_r); orientation - (1) is the same
 * with f and r exchanged; with f == r only + is formed.  A product is kept iff min_len <= end - start <= max_len; every combination
 * counts; a product may span invalid bases and never spans two records.  Without no_threshold a PRIMER site takes part only if its
 * dg <= max_dg (the result must carry a model); probe sites are never filtered.  With a probe p, n_probe of a product is the number
 * of sites of p in that record, on either strand, with end_first <= pos_p and end_p <= pos_last: the probe lies strictly between the
 * two primer sites.  Without a probe n_probe is 0. */
typedef struct sw_amplicons sw_amplicons; /* opaque: the device-resident [n_pairs][n_assemblies] counts of one call, and the products */
/* (no counterpart in the reference)  pairs[n_pairs][2] = (f, r), indices into the call's oligos; probes: NULL, or [n_pairs] with an
 * oligo index or 0xFFFFFFFF (a pair without a probe).  A pair listed twice is two rows.  0 pairs or more than 65 536, an index
 * outside the call's oligos, min_len > max_len, min_len < 1, a result made without sites, no_threshold == 0 on a result without a
 * model: SW_ERR_VALUE before a device is touched.  2^32 products or more (counted in 64 bits): SW_ERR_RUNTIME.  want_products != 0
 * also keeps the list of products.  The result does not depend on `oligos` after the call returns. */
int sw_oligos_amplicons(const sw_oligos *oligos, const uint32_t *pairs, const uint32_t *probes, uint64_t n_pairs, uint64_t min_len,
                        uint64_t max_len, int want_products, int64_t max_dg, int no_threshold, void *stream, sw_amplicons **out);
/* (no counterpart in the reference)  Pairs, assemblies, min_len, max_len of the call (any pointer may be NULL). */
int sw_amplicons_sizes(const sw_amplicons *h, uint64_t *n_pairs, uint64_t *n_assemblies, uint64_t *min_len, uint64_t *max_len);
/* (no counterpart in the reference)  sw_oligos_block for one field: 0 n_amplicons, the products of the pair in the assembly; 1
 * n_detected, those of them with n_probe >= 1 (zero for a pair without a probe). */
int sw_amplicons_block(const sw_amplicons *h, uint64_t field, uint64_t r0, uint64_t r1, uint64_t c0, uint64_t c1, uint32_t *out);
/* (no counterpart in the reference)  Entries of the list of products.  This and sw_amplicons_products: SW_ERR_VALUE for a result made
 * without it. */
int sw_amplicons_products_size(const sw_amplicons *h, uint64_t *n_products);
/* (no counterpart in the reference)  Every product, ascending by (pair, assembly, record, start, end, orientation, mm_f, mm_r) -- rows
 * equal in all eight keep the order (first site, last site) of the site list --: cell_offsets[n_pairs * n_assemblies + 1] and the
 * list's nine columns, n_products entries each.  mm_f / mm_r are d of the site of f / r. */
int sw_amplicons_products(const sw_amplicons *h, uint64_t *cell_offsets, uint32_t *pair, uint32_t *assembly, uint32_t *record, uint32_t *start,
                          uint32_t *end, uint32_t *orientation, uint32_t *mm_f, uint32_t *mm_r, uint32_t *n_probe);
/* (no counterpart in the reference)  counters[6] = { items (first sites offered to a pair and orientation), items on the wave route,
 * partners visited, products, detected products, kernel launches }; ms[3] = { count, emit, order of the list } (HIP events; the last
 * two are 0 without the list). */
int sw_amplicons_stats(const sw_amplicons *h, uint64_t *counters, double *ms);
/* (no counterpart in the reference) */
void sw_amplicons_free(sw_amplicons *h);

/* ---- multi-GPU merge (one process per GPU; the exchange itself is done by the host side with
 *      torch.distributed / RCCL on the device buffers below).  Together these replace
 *      merge_thread_graphs (cpp/src/seqwin/build_internals.cpp:295-392) across GPUs. -------------- */

/* Device addresses of the index arrays (sw_kmer[n_kmers], sw_node[n_nodes], sw_edge[n_edges]). */
int sw_index_device_ptrs(const sw_index *ix, void **kmers, void **nodes, void **edges);
/* Write one row per occurrence, in the index's (hash, record_idx, pos) order, into the caller's DEVICE
 * buffer rows[n_kmers][2] (u64): {node hash, pos | (record_idx + rec_offset) << 32}
 * (record re-basing: build_internals.cpp:334-355, 243-246). */
int sw_index_occ_rows(const sw_index *ix, uint64_t rec_offset, void *rows_dev, void *stream);
/* Copy the edges, as rows[n_edges][3] (u64) = {first, second, weight}, into the caller's DEVICE buffer. */
int sw_index_edge_rows(const sw_index *ix, void *rows_dev, void *stream);
/* For n_bounds ascending hash bounds: occ_split[j] = number of occurrences whose node hash < node_bounds[j];
 * edge_split[j] = number of edges whose `first` < edge_bounds[j] (host outputs). */
int sw_index_splits(const sw_index *ix, const uint64_t *node_bounds, const uint64_t *edge_bounds, uint64_t n_bounds,
                    uint64_t *occ_split, uint64_t *edge_split, void *stream);
/* Build one rank's slice of the merged graph from exchanged rows (DEVICE buffers):
 * occ_rows[n_occ][2] concatenated in source-rank order, edge_rows[n_edge_rows][3] = {first, second, weight}.
 * Node ranges are offset by kmer_base (number of occurrences owned by lower ranks).  record_offsets /
 * is_targets are the GLOBAL host arrays (is_targets may be NULL to skip the counts). */
int sw_index_merge(const void *occ_rows_dev, uint64_t n_occ, const void *edge_rows_dev, uint64_t n_edge_rows,
                   uint64_t kmer_base, const uint32_t *record_offsets, const uint8_t *is_targets,
                   uint64_t n_assemblies, void *stream, sw_index **out);

/* ---- multi-GPU, tuple-exchange form (what bench.py --gpus N times; seqwin_amd/dist.py drives it) ---------
 * Instead of building a partial graph per GPU and merging (above), every GPU sketches its shard and the TUPLES are
 * exchanged by hash range, so each occurrence is sorted exactly once, by its owner:
 *   sw_occ_sketch -> sw_occ_partition -> [all_to_all rows] -> sw_slice_build (nodes / kmers / counts + rank of every
 *   received row) -> [all_to_all ranks back] -> sw_occ_adjacency -> [all_to_all adjacency rows] -> sw_slice_edges. */
typedef struct sw_occ sw_occ; /* device-resident (out_hash, pos|record) stream of one shard in (record_idx, pos) order */
int sw_occ_sketch(const sw_batch *b, uint64_t kmerlen, uint64_t windowsize, void *stream, sw_occ **out);
int sw_occ_size(const sw_occ *o, uint64_t *n, double *sketch_ms);
/* A shard's tuple stream straight from its FASTA files, the files streamed through HBM in chunks of ~chunk_bp bases (0: one
 * chunk) -- low_memory inside a multi-device build (build.cpp:264-325 keeps the peak down by a second pass; here only 16 B per
 * minimizer of a finished chunk stay resident).  *batch_out holds the shard's record tables only (no packed bases). */
int sw_occ_sketch_paths(const char *const *assembly_paths, size_t n_assemblies, uint64_t kmerlen, uint64_t windowsize, uint64_t n_cpu,
                        uint64_t chunk_bp, void *stream, sw_batch **batch_out, sw_occ **occ_out);
void sw_occ_free(sw_occ *o);
/* Stable partition by owner = number of ascending bounds <= out_hash.  DEVICE outputs: rows[n][2] =
 * {out_hash, pos | (record_idx + rec_offset) << 32} grouped by owner, perm[n] (u32: original index of row j; may be
 * NULL -- the handle remembers the partition and sw_occ_adjacency walks it again instead of scattering through perm).
 * HOST output: counts[n_bounds + 1]. */
int sw_occ_partition(const sw_occ *o, const uint64_t *bounds, uint64_t n_bounds, uint64_t rec_offset, void *rows_dev,
                     void *perm_dev, uint64_t *counts, void *stream);
/* Owner: nodes / kmers (+ counts and penalty if is_targets) of its hash range from received rows (concatenated in
 * source-rank order = global (record_idx, pos) order).  ranks_dev[n] (u32, DEVICE) receives the slice-local node rank
 * of every received row.  Node ranges are offset by kmer_base.  The index has no edges yet. */
int sw_slice_build(const void *rows_dev, uint64_t n, uint64_t kmer_base, const uint32_t *record_offsets,
                   const uint8_t *is_targets, uint64_t n_assemblies, void *ranks_dev, void *stream, sw_index **out);
/* Copy the node hashes (u64[n_nodes]) of an index into a DEVICE buffer. */
int sw_index_node_hashes(const sw_index *ix, void *dst_dev, void *stream);
/* Source: adjacency rows of consecutive minimizers of a record, from the GLOBAL node rank of every partitioned row
 * (rank_by_row_dev, u32[n]; perm_dev is only read when the handle was not partitioned by sw_occ_partition and may be NULL
 * otherwise); grouped by edge owner = number of ascending rank_bounds <= rank_lo.
 * asm_bits == 0: DEVICE rows[<= n-1][2] = {(rank_lo << n_bits) | rank_hi, global assembly};
 * asm_bits  > 0 (requires 2 n_bits + asm_bits <= 64): DEVICE rows[<= n-1] = one packed key
 *               (((rank_lo << n_bits) | rank_hi) << asm_bits) | global assembly  -- half the exchange volume.
 * HOST output counts[n_bounds + 1]. */
int sw_occ_adjacency(const sw_occ *o, const void *perm_dev, const void *rank_by_row_dev, uint64_t n_bits,
                     uint64_t asm_bits, uint64_t asm_base, const uint64_t *rank_bounds, uint64_t n_bounds, void *rows_dev,
                     uint64_t *counts, void *stream);
/* Owner: edges of its rank range from received adjacency rows (source-rank order; same format as above), hashes
 * looked up in the job-wide rank -> hash table (DEVICE u64[total nodes]).  Attaches the edges to `ix`. */
int sw_slice_edges(sw_index *ix, const void *adj_rows_dev, uint64_t m, uint64_t n_bits, uint64_t asm_bits,
                   const void *rank_hash_dev, void *stream);

/* ---- the sort primitive of the index stage, on its own (tests, timing) ------------------------------------------------
 * Stable LSD radix sort of n DEVICE u64 keys by bits [begin_bit, end_bit) -- lsd_radix_sort_key
 * (cpp/src/seqwin/build_internals.cpp:76-144) on the device: the hand-written onesweep of csrc/radix.hip (rocPRIM's under
 * SEQWIN_AMD_SORT=rocprim).  keys_dev / alt_dev are a double buffer of n keys each; *sorted_in_alt tells which one holds the
 * result; *ms (may be NULL) the device time. */
int sw_sort_keys64(void *keys_dev, void *alt_dev, uint64_t n, uint64_t begin_bit, uint64_t end_bit, void *stream, int *sorted_in_alt,
                   double *ms);
/* The pair form -- lsd_radix_sort (cpp/src/seqwin/build_internals.cpp:76-110) as the node sort uses it: n DEVICE u32 keys, each
 * with a 16-byte payload, stably by key bits [0, end_bit), end_bit in {8, 16, 24, 32} (csrc/radix.hip's pair passes; rocPRIM's
 * under SEQWIN_AMD_SORT=rocprim or SEQWIN_AMD_PAIR_SORT=rocprim).  Double buffers of n keys / n payloads each. */
/* How the radix passes rank keys inside a wave on the current device: *mode = 1 by one LDS atomic per key -- the device passed
 * the start-up check that the lanes of one LDS atomic are served in lane order (what keeps those passes stable) --, 0 by ballots
 * (the check failed, or SEQWIN_AMD_RADIX_RANK=ballot).  Runs the check if it has not run yet. */
int sw_radix_rank_mode(int *mode);
/* Always-on order guards (r05): the kernels that stream over the sorted occurrences (k_nodes) and the sorted edge keys
 * (k_rle_keys) count every place where (hash, stream index) resp. the key does not ascend -- the stability contract of
 * lsd_radix_sort, cpp/src/seqwin/build_internals.cpp:76-144.  A build that sees such a place logs a WARNING, switches the device
 * to ballot / rocPRIM ranking for the rest of the process and sorts again (bit-identical result).  These counters say how often
 * that happened in this process (0 on a healthy device; SEQWIN_AMD_FAULT_INJECT=rank makes the suite take the path). */
int sw_order_guard_trips(uint64_t *node_sort, uint64_t *edge_sort);
int sw_sort_pairs32(void *keys_dev, void *keys_alt_dev, void *vals_dev, void *vals_alt_dev, uint64_t n, uint64_t end_bit, void *stream,
                    int *sorted_in_alt, double *ms);
/* The bucket route of the edge sort on its own (csrc/radix.hip: radix_edge_buckets, what a single-device build takes from 2^26 edge
 * keys on): m DEVICE u64 keys below 2^key_bits, the value 2^key_bits - 1 being the sentinel of a record boundary; keys_dev /
 * alt_dev are a double buffer of m keys each.  key_bits in [1, 62]; cap: most real keys a sub-bucket may hold (< 2^32); slots: size
 * of the LDS table of a sub-bucket's distinct keys; hist_top_dev: the counts of the keys' top digit (u64[2^digit width], DEVICE) as
 * the producer of the keys takes them, NULL: counted here.
 * *done = 1: ukeys_dev[0, *n_runs) (u64, room for m) holds the distinct real keys in ascending order, ucnt_dev[0, *n_runs] (u32, room
 *            for m + 1) the start of every run of equal keys among the sorted real keys and, last, the number of real keys.
 * *done = 0: the routine declined (fewer than two digits, m = 0 or m >= 2^32 - 1, slots no power of two in [64, 8192], a sub-bucket
 *            above cap real keys or slots distinct keys); nothing else is valid, *n_runs = 0.
 * Either way *keys_in_alt tells which buffer holds the multiset of the input keys afterwards (in some order). */
int sw_edge_buckets(void *keys_dev, void *alt_dev, uint64_t m, uint64_t key_bits, uint64_t cap, uint64_t slots, const void *hist_top_dev,
                    void *ukeys_dev, void *ucnt_dev, uint64_t *n_runs, int *done, int *keys_in_alt, void *stream);

/* ---- pairs form of the adjacency exchange (what dist.py uses whenever every slice marked its ranks) ---------------------
 * The weight of an edge is the number of its adjacency records minus the records that repeat the pair inside one
 * assembly, and only records touching an occurrence whose node occurs more than once in its assembly can do that.  A slice
 * build with a record table and fewer than 2^31 nodes IN THE SLICE marks those occurrences in bit 31 of the slice-local
 * ranks it returns (sw_index_ranks_marked); the sources then send ONE 64-bit key per adjacency record plus the few candidate
 * records with their assembly, and the owners count.
 * Ranks travel slice-LOCAL (32 bits); a source re-bases them itself: global rank = node_base[owner of the tuple] + local
 * rank, which may need more than 32 bits (100 000 random genomes: 5e9 distinct minimizers; the reference indexes nodes with
 * size_t, cpp/include/seqwin/graph.hpp:28-41, cpp/src/seqwin/build_internals.cpp:159-223).  An edge belongs to the owner of
 * its rank_lo's range [lo_base, next lo_base) (rank_bounds), so its key is
 *     (rank_lo - lo_base) << hi_bits | rank_hi,      hi_bits = bits of the total node count, lo_bits = bits of the widest range,
 * lo_bits + hi_bits <= 64 (else SW_ERR_RUNTIME: more GPUs are needed). */
int sw_index_ranks_marked(const sw_index *ix, int *marked);
/* Source: keys_dev[<= n-1] (u64, DEVICE) of every adjacency record, grouped by edge owner (counts[n_bounds + 1]); the candidate
 * records stay in the handle as rows {key, global assembly} grouped by owner (cand_counts[n_bounds + 1]) until
 * sw_occ_candidates copies them (sum of cand_counts rows of 2 u64) to a DEVICE buffer.
 * rank_by_row_dev: slice-local ranks with the repeat mark, in the order of the rows sw_occ_partition wrote (what the reverse
 * all-to-all delivers); node_base[n_owners + 1]: prefix of the node counts of the tuple partition's owners (HOST);
 * rank_bounds[n_bounds]: ascending splitters of the GLOBAL rank space (HOST); key_bits[2] receives {lo_bits, hi_bits}. */
int sw_occ_adjacency_pairs(const sw_occ *o, const void *rank_by_row_dev, const uint64_t *node_base, uint64_t n_owners, uint64_t asm_base,
                           const uint64_t *rank_bounds, uint64_t n_bounds, void *keys_dev, uint64_t *counts, uint64_t *cand_counts,
                           uint64_t *key_bits, void *stream);
int sw_occ_candidates(const sw_occ *o, void *rows_dev, void *stream);
/* Owner: edges of its rank range from the received keys and candidate rows (source-rank order).  keys_dev is sorted in place
 * (its contents are not preserved).  lo_base: first global rank of this owner's range.  rank_hash_dev (DEVICE u64[n_owners * pad]): the job-wide rank -> hash table as
 * all_gather_into_tensor leaves it -- slice owner o's node hashes (sw_index_node_hashes) at [o * pad, o * pad + its count). */
int sw_slice_edges_pairs(sw_index *ix, void *keys_dev, uint64_t m, const void *cand_rows_dev, uint64_t n_cand, uint64_t lo_bits,
                         uint64_t hi_bits, uint64_t lo_base, uint64_t asm_bits, const void *rank_hash_dev, const uint64_t *node_base,
                         uint64_t n_owners, uint64_t pad, void *stream);
/* The same without the job-wide table (rank_hash_dev == NULL above: 8 B per node of the WHOLE job on every GPU -- 40 GB at
 * 5e9 nodes): the edges then hold global ranks and their hashes are asked from the node owners, 12 B per distinct endpoint.
 *   1. edge owner: sw_index_edge_hash_requests -> *n_requests distinct endpoint ranks, as owner-LOCAL ranks (u32) in ascending
 *      global order, counts[n_owners] of them for each node owner; sw_index_edge_hash_request_rows copies them out (DEVICE);
 *   2. the requests travel to the node owners (all-to-all by counts); a node owner answers the ranks it received with
 *      sw_index_node_hash_lookup: hashes_dev[i] = hash of its node local_ranks_dev[i];
 *   3. the replies travel back in request order; sw_index_edge_hash_attach(ix, replies_dev, *n_requests) writes them into the
 *      edges.  Until then sw_index_export / _checksums of this index see ranks in edges.first / .second. */
int sw_index_edge_hash_requests(sw_index *ix, const uint64_t *node_base, uint64_t n_owners, uint64_t *counts, uint64_t *n_requests,
                                void *stream);
int sw_index_edge_hash_request_rows(const sw_index *ix, void *local_ranks_dev, void *stream);
int sw_index_node_hash_lookup(const sw_index *ix, const void *local_ranks_dev, uint64_t n, void *hashes_dev, void *stream);
int sw_index_edge_hash_attach(sw_index *ix, const void *replies_dev, uint64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SEQWIN_HIP_H */
