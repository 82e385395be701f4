/* halo2hip_debug.h -- test and tuning hooks of libhalo2hip.so.
 *
 * Not part of the drop-in surface (include/halo2hip.h): nothing a halo2 prover calls.  tests/ and tools/ reach these
 * through ctypes to force code paths (chunking, window widths, kernel variants) and to sweep tuning constants.
 *
 * The settings are process-wide and survive h2hip_shutdown.  A setter (h2hip_debug_set_*, h2hip_set_msm_window) may be called from
 * any thread at any time: it waits for the calls that are running and takes effect from the next one.  It needs no GPU and does
 * not start the engine.  It must not be called from inside a callback of the library (it would wait for the call it is in).
 * Where a setter says "0 restores the default", the default is the one written at the setting's member of `struct Tuning`
 * (csrc/engine.h) and is not repeated here; a value stated below is one the caller has to pass to get the default back.
 */
#ifndef HALO2HIP_DEBUG_H
#define HALO2HIP_DEBUG_H
#include "halo2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a host-resident MSM of at least min_n pairs streams across PCIe in `chunks` pieces (1 = off; 0 = by size: three, two below 2^20
 * pairs) whose sizes grow by 1000 / ratio_permille (upload time over compute time per pair); with the bases crossing too
 * (unpinned) twice the chunks at twice the ratio; zeros restore the defaults */
int h2hip_debug_set_msm_stream(uint32_t chunks, uint32_t ratio_permille, size_t min_n);
/* needs no GPU: the chunk sizes a streamed MSM of n pairs is cut into (0 = the values in force); returns their number */
size_t h2hip_debug_msm_stream_ladder(size_t n, uint32_t chunks, uint32_t ratio_permille, int with_bases, size_t* sizes, size_t cap);
/* split MSM inputs above m pairs into consecutive chunks (0 restores the default, the 31-bit pair-index limit) */
int h2hip_debug_set_msm_max_chunk(size_t m);
/* push `count` Jacobian partials per engine device through the library's RCCL all-gather (communicators created on
 * demand, also for one device) and fold them on the host: exercises the multi-GPU gather on any box */
int h2hip_debug_rccl_gather_selftest(const uint64_t* partials_xyz, size_t count, uint64_t* out_xyz);
/* record form of the window tables built by h2hip_bases_pin* from now on (read at pin time): 64 = E-form points as the reference stores them,
 * 80 or 128 = the multiplier's own limb form (80 bytes) at that stride; 0 = the engine's choice (128 from 2^13 points, where its memory
 * rules allow the larger table; 64 otherwise).  h2hip_bases_pinned_info reports the bytes the table really takes. */
int h2hip_debug_set_table_records(uint32_t bytes);
/* buckets with more than (entries of the MSM) / d entries take the chunked path (0 restores the default) */
int h2hip_debug_set_msm_heavy_div(size_t d);
/* g_to_lagrange / fft_g1 up to k = 14: bit 0 -- one quad of lanes per butterfly (1, default) or one lane (0); bit 1 set -- normalise to affine
 * after every layer as round 3 did (default clear: the points stay XYZZ between the layers, one normalisation at the end) */
int h2hip_debug_set_g2l_quad(int on);
/* fused batches: at most `entries` entries per fused run, MSMs of at most `max_n` pairs are fused (0 restores a default) */
int h2hip_debug_set_msm_fuse_limits(size_t entries, size_t max_n);
/* first row/column pass of the reduction: lane budget (0 restores the default, one wave per SIMD) */
int h2hip_debug_set_msm_rowcol(uint64_t lanes);
/* accumulation of runs with fewer than 2^18 buckets: up to 8 lanes per bucket (1, default) or one (0) */
int h2hip_debug_set_msm_split_buckets(int on);
/* runs with at most 4 bucket sets: finish the reduction on the host from bit-plane sums (1, default) or keep the GPU tail (0) */
int h2hip_debug_set_msm_plane_tail(int on);
/* reduction tail: one quad of lanes per group operation (1, default) or one lane each (0) */
int h2hip_debug_set_msm_quad_tail(int on);
/* needs no GPU: the geometry of the bucket reduction of one run of `fuse` MSMs of n pairs each under the settings in force; table_c = 0 is
 * the plain form, otherwise the fixed-base form over a window table of that width.  out[0..13) = n_sets, cb, levels, s, rb, s2, s3,
 * split_log, heavy_t, tail (0 = lane, 1 = quad, 2 = bit planes finished on the host), c, W, entries per heavy chunk; out[13] = the
 * row/column jobs that run and out[14..] the g_log of each in launch order (first pass: rows, columns; second pass: RR, RC, CR, CC).
 * Returns the plan's length in words (what lies beyond cap is not written), or -1 for a run the engine refuses */
int h2hip_debug_msm_reduce_plan(size_t n, uint32_t fuse, uint32_t table_c, uint32_t* out, size_t cap);
/* level-1 sort records of runs whose bins span several level-2 tiles: entries and key bits as two arrays (1, default) or 8-byte pairs (0) */
int h2hip_debug_set_msm_split_records(int on);
/* target entries per coarse bin of the MSM's two-level sort (0 restores the default) */
int h2hip_debug_set_msm_bin_entries(size_t d);
/* batches of MSMs of up to 2^19 pairs: fused into one run (1, default) or pipelined over streams (0) */
int h2hip_debug_set_msm_fuse_small(int on);
/* largest log2 tile of an NTT pass (clamped to 4..10; no reset value: the default is 8, which takes 9 beyond 2^24 points) */
int h2hip_debug_set_ntt_smax(uint32_t v);
/* needs no GPU: the plan an NTT of `count` columns of 2^log_n points takes under the settings in force -- returns its number of passes
 * (1..4; the two-pass plan of 2^19..2^22 reports 2) and fills radices[0 .. passes) with the log2 tile of each pass, first pass first;
 * -1 for log_n > 28 or a null array */
int h2hip_debug_ntt_plan(uint32_t log_n, size_t count, uint32_t radices[4]);
/* HALO2_HIP_LAZY_PIN without the environment: a host bases array seen `after` times unpinned is pinned by the library (0 = never, the default) */
int h2hip_debug_set_lazy_pin(uint32_t after);
/* sizes 2^lo..2^hi take the two-pass plan (hi < lo: never; 0, 0: back to the defaults) */
int h2hip_debug_set_ntt_two_pass(uint32_t lo, uint32_t hi);
/* HALO2_HIP_NTT_TWIDDLE_MB in bytes: HBM per device the full inter-pass twiddle tables may take (0 = none: the two-level table only; no
 * reset value: the default is 4 GB) */
int h2hip_debug_set_ntt_twiddle_budget(uint64_t bytes);
/* batched transforms: bytes of columns + workspace one launch spans (0 restores the default) */
int h2hip_debug_set_ntt_batch_bytes(uint64_t bytes);
/* two-pass plan for batched columns of 2^17 / 2^18 points: from this many pairs of workgroups per pass (0 restores the default) */
int h2hip_debug_set_ntt_two_pass_batch_wgs(uint64_t v);
/* three-pass plan: strided passes up to 2^v points read their inter-pass twiddles from a per-domain table (0 restores the default) */
int h2hip_debug_set_ntt_full_max_log_m(uint32_t v);
/* 0: no scaled copies of the inter-pass tables (the inverse's 1/n is then a multiplication in the last pass); 1 = default */
int h2hip_debug_set_ntt_fold_tables(int on);
/* host-pointer batched transforms: device bytes one pipelined run may hold (smaller forces several runs) and the size below which
 * columns are grouped per pipeline step; 0 restores a default */
int h2hip_debug_set_ntt_host_batch(uint64_t run_bytes, uint64_t group_bytes);
/* two-pass plan: log2 columns per workgroup (-1 = default) */
int h2hip_debug_set_ntt_two_pass_log_j(int v);
/* evaluate_h: programs needing more slots than v use the global-workspace form of the kernels (no reset value: the default is 256) */
int h2hip_debug_set_evalh_max_local_slots(uint32_t v);
/* evaluate_h: HBM one group of lookup cosets may take (0 restores the default; the first group is transformed with the advice columns) */
int h2hip_debug_set_evalh_lookup_group_bytes(uint64_t v);
/* evaluate_h: field multiplications per row of the program a graph compiles to; needs no GPU */
int h2hip_debug_evalh_program_muls(const h2hip_graph* g, uint32_t* n_mul);
/* evaluate_h: the kernels generated per circuit (hiprtc) -- the custom gates', one per halo2 lookup and, where the stage's are wanted, one
 * per shuffle and per mv-lookup argument.  mode bits 0-3: 0 off, 1 compiled on a background thread while the interpreter serves (default;
 * HALO2_HIP_EVALH_CODEGEN takes the same number), 2 compiled inline; + 16: without the fusion of two products into one reduction; the two-bit
 * field at + 32 / + 64 selects the shuffle and mv-lookup kernels: 0 the default set (`struct Tuning`), + 32 none (gates and lookups keep
 * theirs), + 64 both.  max_ops: kernels with more operations over all their programs (or more than 48 values alive at once) stay with the
 * interpreter (0 restores the default).  (1, 0) restores every default. */
int h2hip_debug_set_evalh_codegen(int mode, uint32_t max_ops);
/* the HIP source a graph's program is emitted as (buf may be NULL: *len alone), and with bit 0 of `compile` set what hiprtc makes of it for
 * gfx950 (seconds, bytes of code object); bit 1: the graph as a lookup argument's table expression (evalh_lookup_gen) instead of the custom
 * gates (evalh_gates_gen); needs no GPU.  Returns 0, 1 (malformed graph) or 2 (hiprtc missing / rejected the source). */
int h2hip_debug_evalh_codegen_source(const h2hip_graph* g, char* buf, size_t cap, size_t* len, int compile, double* seconds, size_t* code_bytes);
/* ... and the source of a stage kernel, one kernel from several programs: kind 1 = a shuffle (n_graphs == 2: the input side's graph, then the
 * shuffle side's; evalh_shuffle_gen), kind 2 = an mv-lookup argument (n_graphs == K + 1: the K input tuples' graphs, then the table's;
 * evalh_mvlookup_gen).  Host only.  Returns 0, 1 (malformed input: a bad kind or count, a malformed graph, a graph reading a value the stage
 * does not supply), 2 (hiprtc missing / rejected the source) or 3 (the kernel is beyond the generator's limits -- operations over all
 * programs, values alive at once -- and the engine would keep the interpreter; *len = 0). */
int h2hip_debug_evalh_codegen_stage_source(const h2hip_graph* graphs, uint32_t n_graphs, int kind, char* buf, size_t cap, size_t* len, int compile,
                                           double* seconds, size_t* code_bytes);
/* out: kernels compiled, compilations failed, launches of a generated kernel, launches of the interpreter, disk-cache hits.  compiled,
 * failed and disk hits count every generated kernel, the shuffles' and mv-lookups' included; the two launch counts are the gates' and
 * the halo2 lookups' alone, as they were before those stages had kernels (h2hip_debug_evalh_codegen_stage_stats has every stage's). */
int h2hip_debug_evalh_codegen_stats(uint64_t out[5]);
/* out[0 .. 8): launches of a generated kernel, then of the interpreter, for the gates, the halo2 lookups, the shuffles and the mv-lookups in
 * that order; out[8]: background compilations queued or running (a stage kernel is queued only while fewer than 8 are) */
int h2hip_debug_evalh_codegen_stage_stats(uint64_t out[9]);
/* evaluate_h: compile a graph as the engine would and report the program's size; needs no GPU */
int h2hip_debug_evalh_compile_stats(const h2hip_graph* g, uint32_t* n_ops, uint32_t* n_slots);
/* evaluate_h: the program a graph compiles to; needs no GPU.  *n_ops, *n_slots and result (kind, a, b of the value the row stores; kind 11 =
 * the field's zero, an empty graph) are always filled; with cap_ops >= *n_ops also, per op and where the pointer is not NULL: ops = 8 words
 * (op with the reduce flag 0x100, dst slot, x.kind, x.a, x.b, y.kind, y.a, y.b; an INTERMEDIATE operand's a is its slot), mags = the
 * magnitude in units of r that the compiler tracked for the op's result (after its reduction where it carries one), fused_on / fused_off =
 * the op inside which the per-circuit generator emits this product (two products meeting in a sum share one reduction), or -1, with the
 * fusion on (the default) and off (h2hip_debug_set_evalh_codegen mode + 16).  Returns 0 or 1 (malformed graph, null argument). */
int h2hip_debug_evalh_program(const h2hip_graph* g, uint32_t* ops, size_t cap_ops, uint32_t* n_ops, uint32_t* n_slots, uint32_t result[3],
                              double* mags, int32_t* fused_on, int32_t* fused_off);
/* the split of a domain's two-level power table (omega^e = lo[e & (2^lo_bits - 1)] * hi[e >> lo_bits]) that evaluate_h's permutation
 * kernel walks: rows at or beyond 2^lo_bits take the second factor.  Builds the table when the domain has none yet; needs a GPU. */
int h2hip_debug_evalh_power_table_bits(const uint64_t omega[4], uint32_t log_n, uint32_t* lo_bits);
/* the last h2hip_evaluate_h_parts_bn254[_device] call of the calling thread: out[0] = columns scaled and transformed, summed over the
 * call's parts; out[1] = columns served from pinned part cosets, summed over parts; out[2] = column bytes uploaded (host form; `values`
 * not counted); out[3] = arena bytes taken behind the metadata */
int h2hip_debug_evalh_parts_stats(uint64_t out[4]);
/* A/B: 1 = the parts form scales its unpinned columns inside the transform's first-pass load (as h2hip_coeff_to_extended_part_* always
 * does); 0 = with the scale kernel in front of a plain transform (default) */
int h2hip_debug_evalh_part_fused(int on);
/* opening (evaluations and combine / divide): force the tile shape, consecutive rows per thread (power of two <= 64) and threads per
 * tile (power of two <= 256), so that small inputs span many tiles; 0 restores the size-based default. */
int h2hip_debug_set_opening_tile(uint32_t rows_per_thread, uint32_t threads_per_tile);
/* lookup permutation: force the in-LDS sort block (a power of two in [4, 1024]; 0 = the kernel's tile) so that small columns run the merge
 * passes.  Stats: out[0] = the block and out[1] = the merge passes (log2(2^k / block)) of the last permute call. */
int h2hip_debug_set_lookup_sort(uint32_t lds_keys);
int h2hip_debug_lookup_sort_stats(uint32_t out[2]);
/* keygen: the HBM one group of columns of a host-pointer h2hip_permutation_keygen_bn254 / h2hip_batch_invert_assigned_bn254 call may take
 * (0 restores the default), so that small inputs run several pipelined groups. */
int h2hip_debug_set_keygen_group(uint64_t group_bytes);
/* randomness: the element count from which the host forms of h2hip_fr_random_bn254 / h2hip_fr_from_bytes_wide_bn254 go to the device
 * (1: always; SIZE_MAX: never, the calling thread's loop at any n; 0 restores HALO2_HIP_RANDOM_MIN_N or the default). */
int h2hip_debug_set_random_min_n(size_t n);
/* mv-lookup grand sum: the consecutive rows one thread of the scan takes in a call of `count` arguments at this k and blinding_factors --
 * the rule h2hip_mvlookup_sums_bn254 itself applies (the grand products' rule).  Needs no GPU. */
int h2hip_debug_mvlookup_sum_rows(uint32_t k, uint32_t blinding_factors, size_t count, uint32_t* rows);
/* permutation mapping from copies: the sort of a call with n_copies copies -- out[0] = the keys one workgroup sorts in LDS (the block: the
 * 2 n_copies endpoint keys are padded to a multiple of it), out[1] = the merge passes that follow.  The block is fixed (no setter: tests
 * choose their copy counts around it).  Needs no GPU. */
int h2hip_debug_copies_sort_plan(size_t n_copies, uint32_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* HALO2HIP_DEBUG_H */
