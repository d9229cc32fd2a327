/*
 * whatshap_amd_debug.h -- TEST INFRASTRUCTURE, not part of the drop-in boundary.
 *
 * Entry points that exist only in libwhatshap_amd_debug.so (the product sources compiled with -DWHAMD_DEBUG_BUILD, `make debug`):
 * CPU emulators of the run plans and the single-thread host instantiation of the heuristic, which the CPU test-suite compares with
 * the oracle.  The debug library also carries the kernel instantiations with in-kernel cycle stamps and the timing switches
 * (WHAMD_SLOT_STAMPS, WHAMD_SLOT_SKIP: results invalid) that scripts/gpu_slot_*.py use.  libwhatshap_amd.so has none of this.
 */
#ifndef WHATSHAP_AMD_DEBUG_H
#define WHATSHAP_AMD_DEBUG_H

#include "whatshap_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only diagnostic of the slot-run planner (no device needed, small inputs only): builds the forward plan of a
 * single-individual table exactly as whamd_dptable_create would (slot_l local slots preferred -- add 100 for 8 instead of 4 cells per thread --, symmetry level) and
 * executes it cell by cell on the CPU the way the kernels do -- same physical cell indices, decision bits, record
 * layout, exchange layouts and mirror rules.  index_out[n_columns]: the index path (index_path[c].index,
 * src/pedigreedptable.h:17-21), score_out: the optimal score.  Lets the CPU test-suite check the PLAN against the
 * oracle; not a solver and never used by one (WHAMD_ERR_UNSUPPORTED for pedigrees). */
whamd_status_t whamd_debug_emulate_slot_plan(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                            const whamd_pedigree_view* pedigree, int distrust_genotypes,
                                            const uint32_t* positions, size_t n_positions, int slot_l, int symmetry,
                                            uint32_t* index_out, uint32_t* score_out, uint64_t* n_run_columns_out);

/* The same diagnostic for a pedigree table with one or two trios (T = 4 / 16): the pedigree slot plan (one (cell,
 * transmission value) per lane, cost forms split into per-workgroup / per-wave / per-lane tables, butterfly min-plus
 * step, one record byte per lane and column) executed on the CPU as kernels_pedslots.h does it.  slot_l <= 0: the
 * default number of local slots, else that many.  transmission_out[n_columns]: index_path[c].inheritance_value.
 * WHAMD_ERR_UNSUPPORTED when the table is not eligible for pedigree slot runs. */
whamd_status_t whamd_debug_emulate_pedslot_plan(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                               const whamd_pedigree_view* pedigree, int distrust_genotypes,
                                               const uint32_t* positions, size_t n_positions, int slot_l,
                                               uint32_t* index_out, uint32_t* transmission_out, uint32_t* score_out,
                                               uint64_t* n_run_columns_out);

/* Host-only check of the LAZY generic term lists (csrc/problem.cpp build_problem `lazy_fact_terms` + fill_lazy_terms: what whamd_dptable_create does for a
 * trio / quartet with untrusted genotypes whose runs read the factorised line): the problem is built twice -- every term list at once, and lazily with the
 * lists of the columns whose bit is set in need[n_columns] (NULL: every column) filled in afterwards, in `rounds` calls (the columns dealt out round robin) --
 * and the two are compared term by term on the needed columns.  *lazy_out: 1 if the table took the lazy route at all (0: not a factorised table, nothing to
 * compare); *differences_out: columns whose lists differ (0 expected); *built_before_out / *built_after_out: columns with term lists before / after the fills. */
whamd_status_t whamd_debug_lazy_terms_check(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                            const whamd_pedigree_view* pedigree, int distrust_genotypes,
                                            const uint32_t* positions, size_t n_positions, const uint8_t* need, int rounds,
                                            int* lazy_out, uint64_t* differences_out, uint64_t* built_before_out, uint64_t* built_after_out);

/* HOST-ONLY DIAGNOSTIC: the same solver source run with one CPU thread (csrc/heuristic_host.cpp), for the CPU test-suite to
 * compare with the compiled reference; never what the drop-in class calls. */
whamd_status_t whamd_debug_pedmec_heuristic_create_host(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                                        const whamd_pedigree_view* pedigree, int distrust_genotypes,
                                                        const uint32_t* positions, size_t n_positions, uint32_t row_limit, int allow_mutations,
                                                        whamd_heuristic** out);

/* HOST-ONLY DIAGNOSTIC of allele detection (csrc/realign.cpp): the same CIGAR walk as whamd_realign_detect, then both distances and the
 * decision restated on one CPU thread -- the cross-check the CPU test-suite compares with the reference's recorded yields; never what
 * the product calls.  The handle is read with the whamd_realign_* getters of the debug library. */
whamd_status_t whamd_debug_realign_detect_host(const whamd_realign_alignments_view* alignments, const whamd_realign_variants_view* variants,
                                               const whamd_realign_reference_view* reference, const whamd_realign_params* params,
                                               whamd_realign** out);
/* whamd_edit_distance_batch on the host (same restatement as above). */
whamd_status_t whamd_debug_edit_distance_host(uint64_t n_pairs, const uint64_t* query_ptr, const uint8_t* query, const uint64_t* target_ptr,
                                              const uint8_t* target, int use_affine, const float* mismatch_cost, int32_t gap_start,
                                              int32_t gap_extend, int64_t* distance_out);

/* THE LAUNCH SHAPE of realign's long jobs (csrc/realign_shape.h, DESIGN.md: the table of shapes): what the second launch of
 * whamd_realign_detect / whamd_edit_distance_batch -- the one over the jobs whose query is longer than 64 -- looks like for n_long such jobs
 * whose longest allele window (target) is max_target bytes.  Host code, no device needed.  blocks = 0: no second launch.  lds_bytes: dynamic
 * LDS per workgroup (affine strip boundary rows in LDS); scratch_bytes: global scratch (unit carry rows of carry_words words per lane, or
 * affine rows of row_floats floats per wave when global_rows = 1). */
typedef struct whamd_debug_realign_shape {
	uint32_t blocks, block;
	uint64_t lds_bytes, scratch_bytes;
	uint32_t carry_words, row_floats;
	int32_t global_rows, reserved;
} whamd_debug_realign_shape;
whamd_status_t whamd_debug_realign_long_shape(int use_affine, uint64_t n_long, uint32_t max_target, whamd_debug_realign_shape* out);
/* What the shape of a call is made from: the host walk of whamd_realign_detect on the same views (jobs, long jobs, the longest allele window
 * of a long job), and the same two counts for the pairs of a whamd_edit_distance_batch.  Any out pointer may be NULL. */
whamd_status_t whamd_debug_realign_walk_counts(const whamd_realign_alignments_view* alignments, const whamd_realign_variants_view* variants,
                                               const whamd_realign_reference_view* reference, const whamd_realign_params* params,
                                               uint64_t* n_jobs_out, uint64_t* n_long_out, uint32_t* max_target_long_out);
whamd_status_t whamd_debug_edit_distance_long_counts(uint64_t n_pairs, const uint64_t* query_ptr, const uint64_t* target_ptr, uint64_t* n_long_out,
                                                     uint32_t* max_target_long_out);

/* HOST-ONLY DIAGNOSTIC of polyphase read scoring (csrc/polyscore.cpp): the same matrices, term tables and windows as whamd_poly_score,
 * then the pair loop on one CPU thread with the device's arithmetic -- the device's bit-exact reference and what the CPU test-suite
 * compares with the recorded reference; never what the product calls.  Read with the whamd_poly_score_* getters of the debug library. */
whamd_status_t whamd_debug_poly_score_host(const whamd_poly_matrix_view* matrices, uint64_t n_matrices, uint32_t min_overlap, uint32_t ploidy,
                                           double err, whamd_poly_scores** out);

/* HOST-ONLY DIAGNOSTICS of progeny marker scoring (csrc/progeny.cpp): the same entry lists as whamd_progeny_score, then the pair loop on
 * one CPU thread on the caller's table with the device's inner function -- what the CPU test-suite holds to the recorded reference bit for
 * bit; never what the product calls.  Read with the whamd_progeny_score_* getters of the debug library. */
whamd_status_t whamd_debug_progeny_score_host(const whamd_progeny_view* problems, uint64_t n_problems, whamd_progeny_scores** out);
/* The same for a caller-given list of pairs of one problem (a sample of a large one): stored_out[x] = 1 and score_out[x] where the
 * reference's loop stores an entry for (i[x], j[x]), else 0. */
whamd_status_t whamd_debug_progeny_score_entries_host(const whamd_progeny_view* problem, uint64_t n_entries, const uint32_t* i, const uint32_t* j,
                                                      double* score_out, uint8_t* stored_out);
/* One pair score of the table: kind 0 getSimplexNulliplexScore, 1 getSimplexSimplexScore, 2 getDuplexNulliplexScore (pos1, pos2). */
whamd_status_t whamd_debug_progeny_pair_score_host(const float* gl, uint64_t n_positions, uint32_t n_samples, uint32_t ploidy, uint64_t pos1,
                                                   uint64_t pos2, uint32_t kind, double* score_out);
/* whamd_progeny_variant_types on one CPU thread. */
whamd_status_t whamd_debug_progeny_variant_types_host(const float* gl, uint64_t n_positions, uint32_t n_samples, uint32_t ploidy, const double* priors,
                                                      const uint32_t* nodes, uint64_t n_nodes, double* llh_out, uint32_t* g0_out, uint32_t* g1_out);
/* whamd_progeny_gl on one CPU thread: the same validation, then csrc/progeny.h's cell function -- the code the kernel runs -- per cell. */
whamd_status_t whamd_debug_progeny_gl_host(const whamd_progeny_depths_view* problems, uint64_t n_problems, float* const* table_out,
                                           double* const* table_f64_out);

/* HOST-ONLY DIAGNOSTICS of haplotagging (csrc/haplotag.cpp): the same validation and grouping as whamd_haplotag, then every group scored on
 * one CPU thread with the device's selection functions -- what the CPU test-suite holds to the recorded reference, identical in every
 * field; never what the product calls.  Read with the whamd_haplotag_* getters of the debug library. */
whamd_status_t whamd_debug_haplotag_host(const whamd_haplotag_view* problems, uint64_t n_problems, whamd_haplotag_result** out);

/* HOST-ONLY DIAGNOSTICS of polyphase reordering (csrc/polyreorder.cpp): the same validation, windows and read lists as whamd_poly_reorder,
 * then the left / right table and every permutation's sum on one CPU thread with the functions the kernels call (csrc/polyreorder.h) --
 * what the CPU test-suite holds to the recorded reference, bit for bit; never what the product calls.  Read with the
 * whamd_poly_reorder_* getters of the debug library. */
whamd_status_t whamd_debug_poly_reorder_host(const whamd_poly_reorder_view* problems, uint64_t n_problems, double log_match, double log_err,
                                             whamd_poly_reorder_result** out);

/* HOST-ONLY DIAGNOSTICS of comparing polyploid phasings (csrc/polycompare.cpp): the same validation as whamd_poly_compare, then every job
 * state by state on one CPU thread with the functions the kernel calls (csrc/polycompare.h) -- bit-identical to the device, launches
 * nothing; what the CPU test-suite holds to the recorded reference.  Read with the whamd_poly_compare_* getters of the debug library. */
whamd_status_t whamd_debug_poly_compare_host(const whamd_poly_compare_view* jobs, uint64_t n_jobs, whamd_poly_compare_result** out);

/* HOST-ONLY DIAGNOSTICS of haplotagphase (csrc/tagphase.cpp): the same validation as whamd_tagphase, then every vote on one CPU thread
 * with the device's selection function (csrc/tagphase.h) -- what the CPU test-suite holds to the recorded reference, identical in every
 * field; never what the product calls.  Read with the whamd_tagphase_* getters of the debug library. */
whamd_status_t whamd_debug_tagphase_host(const whamd_tagphase_view* problems, uint64_t n_problems, whamd_tagphase_result** out);

/* HOST-ONLY DIAGNOSTICS of the prior genotype likelihoods (csrc/priorgt.cpp): the same validation and mapping as whamd_prior_genotypes,
 * then every column's chain and tail on one CPU thread with the functions the kernel calls (csrc/priorgt.h) -- what the CPU test-suite
 * holds to the recorded reference, bit for bit; never what the product calls.  Read with the whamd_prior_genotypes_* getters of the
 * debug library. */
whamd_status_t whamd_debug_prior_genotypes_host(const whamd_prior_genotypes_view* problems, uint64_t n_problems, whamd_prior_genotypes_result** out);

/* HOST-ONLY DIAGNOSTICS of the read merging (csrc/readmerge.cpp): the same validation, packing and partner ranges as whamd_readmerge,
 * then every pair and every sum in plain loops on one CPU thread with the functions the kernels call (csrc/readmerge.h) -- what the CPU
 * test-suite holds to the recorded reference, the same bytes as the device; never what the product calls.  Launches nothing.  Read with
 * the whamd_readmerge_* getters of the debug library. */
whamd_status_t whamd_debug_readmerge_host(const whamd_readmerge_view* problems, uint64_t n_problems, whamd_readmerge_result** out);

/* THE LAUNCH LEDGER (csrc/dp_device.hip): which kernel instantiation every launch of a solve took, so that a test can hold the
 * choice itself -- not only the result -- against the rules of DESIGN.md 6.2 and slots.h.  Host code of the debug library only.
 *
 * The registry: every kernel a solve can launch, under the spelling of its instantiation ("slot_run<3, false, true, true>").
 * large_lds_opted_in: the kernel is in the array the large-LDS opt-in walks (a launch with more than 64 KiB of dynamic LDS needs it);
 * debug_only: an instantiation only this library has (cycle stamps, timing switches, pedigree X runs). */
typedef struct whamd_debug_kernel {
	const void* kernel;
	const char* name;
	int32_t large_lds_opted_in;
	int32_t debug_only;
} whamd_debug_kernel;
/* Writes at most `capacity` entries to out[] (may be NULL) and returns how many there are. */
size_t whamd_debug_solve_kernels(whamd_debug_kernel* out, size_t capacity);

/* Where a launch was made. */
enum {
	WHAMD_LAUNCH_COLUMN = 0,      /* launch_column_step: column_step_fused | column_step_keys / column_step_wide + column_finalize */
	WHAMD_LAUNCH_RUN = 1,         /* launch_run: an LDS-resident run on its own */
	WHAMD_LAUNCH_SLOT_RUN = 2,    /* launch_slot_run: a slot run on its own */
	WHAMD_LAUNCH_BATCH = 3,       /* submit_super_step: the runs of a super-step as one resident_batch / slot_batch launch */
	WHAMD_LAUNCH_GROUP = 4,       /* GroupSubmission::flush: one variant's runs of several tables */
	WHAMD_LAUNCH_GROUP_WALK = 5,  /* GroupSubmission::walk_batch: the batched backtrace and superreads */
	WHAMD_LAUNCH_TAIL = 6,        /* submit_tail: backtrace and superreads of one table */
	WHAMD_LAUNCH_WINDOW_WALK = 7, /* submit_super_step: the walk of one window of a windowed solve */
	WHAMD_LAUNCH_TABLES = 8       /* begin_solve: ped_tables / resident_tables */
};

/* One line of a table's ledger: `count` launches that agree in everything else.  A fact the launch site does not have is -1.  A launch of a group
 * is entered in every member that counts it in whamd_solve_stats::forward_launches. */
typedef struct whamd_debug_launch {
	const void* kernel;
	uint32_t site;          /* WHAMD_LAUNCH_* */
	uint32_t grid_x, grid_y, block;
	uint32_t lds;           /* dynamic LDS bytes */
	uint32_t own_stream;    /* 1: the table's own stream, 0: the stream of a group's lead */
	uint32_t forward;       /* 1: counted in forward_launches */
	/* what the choice was made from */
	int32_t lr, yflags, spec, stamps, tb, nf, ncols, threads;   /* of a run launched on its own (run.threads ...) */
	int32_t streamed, pack;                                     /* X runs */
	int32_t tight, variant;                                     /* group launches: GroupVariant */
	int32_t T, n_ind, mode, wide;                               /* per-column steps */
	int32_t ped, sym;                                           /* LDS-resident runs: sg.kind, the complement symmetry */
	int32_t entries;                                            /* runs of a batched launch */
	int32_t preview;        /* 1: the launch was made by whamd_dptable_create (the table's preview), 0: by the solve */
	int32_t reserved;
	uint64_t count;
	const char* name;       /* the registry's name of `kernel`; NULL: the pointer is not registered (an error of the library) */
} whamd_debug_launch;
/* The ledger of the solve the table collected last (after whamd_dptable_wait): at most `capacity` lines to out[] (may be NULL), *n_out: how many there are. */
whamd_status_t whamd_debug_dptable_launches(const whamd_dptable* table, whamd_debug_launch* out, size_t capacity, size_t* n_out);

/* THE PREVIEW of a table (options `preview`, `preview_pieces` of whatshap_amd.h): what became of it.
 * ran: whamd_dptable_create launched the table's leading slot runs; pieces: the plan pieces they cover; launched_steps: how many super-steps;
 * agreed_steps: S, the leading super-steps of the finished schedule that are launch for launch what was launched; continued: the solve in flight or
 * collected last began behind the preview (only when S == launched_steps); from_hook: 1 when the launches went out from the planner's head hook (in front of
 * the plan's second half), 0 when behind the whole plan; why_not: "" when it ran, else a line that starts "no preview: ".
 * WHAMD_PREVIEW_MISMATCH_AT=k (environment, this library only) makes the comparison report that step k differs. */
typedef struct whamd_debug_preview {
	int32_t ran, continued;
	uint32_t pieces, launched_steps, agreed_steps, from_hook;
	const char* why_not;
} whamd_debug_preview;
whamd_status_t whamd_debug_dptable_preview(const whamd_dptable* table, whamd_debug_preview* out);

/* HOST-ONLY check of what a preview works out ahead of the create (no device needed): the plan of a single-individual table as whamd_dptable_create makes it, the
 * preview forced over `pieces` plan pieces (0: the library's rule), then the create's own host phases.  For the preview's steps k < steps (at most `capacity` are
 * written; any array may be NULL): the record offset and the seed id the preview would launch step k with, and the ones the create's layout gives the same run.
 * The scalars: what the preview predicts for the whole table beside what the create computes -- arena bytes, the seeds' count and stride, whether the backtrace is
 * chunked, and the bytes of an exchange column (the preview's is a bound: at least the create's).  Free HBM is taken as 1 TiB. */
typedef struct whamd_debug_preview_plan_result {
	uint32_t n_pieces, pieces, steps, n_steps;   /* plan pieces of the table; pieces and leading steps of the preview (0 steps: none, see why_not); steps of the whole plan */
	int32_t chunked_predicted, chunked, windowed, reserved;
	uint32_t n_seeds_predicted, n_seeds, stride_predicted, stride;
	uint64_t arena_predicted, arena_laid_out, exchange_predicted, exchange_laid_out;
	const char* why_not;
} whamd_debug_preview_plan_result;
whamd_status_t whamd_debug_preview_plan(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                        const whamd_pedigree_view* pedigree, int distrust_genotypes,
                                        const uint32_t* positions, size_t n_positions, uint32_t pieces, whamd_debug_preview_plan_result* out,
                                        uint64_t* rec_predicted, uint64_t* rec_laid_out, uint32_t* spec_predicted, uint32_t* spec_laid_out, size_t capacity);

/* HOST-ONLY check of the planner's head hook (csrc/slots.h SlotPlanHead; no device needed): the slot plan of a single-individual table as whamd_dptable_create
 * makes it, with the head -- the leading slot runs inside the first `head_pieces` plan pieces -- finished first (head_pieces = 0: without the hook, one pass).
 * digest: a hash over the finished plan (steps, runs, the rows and backtrace columns of every run, control words, ending and starting slots, their offsets, exit
 * slots, the component list): equal for every head_pieces exactly when the plans are.  head_digest_in_hook: the same hash over the head's part (runs [0, head_steps),
 * their rows, control words, ending slots and backtrace columns) taken INSIDE the callback; head_digest: over the same part of the finished plan.  hook_calls: how
 * often the callback was made.  edge_yflags: SlotRun::yflags of the last run of the head and of the first step behind it (0xFFFFFFFF: not a run, or no head). */
typedef struct whamd_debug_head_plan_result {
	uint32_t n_pieces, head_steps, n_steps, hook_calls;
	uint64_t digest, head_digest_in_hook, head_digest;
	uint32_t edge_yflags[2];
	uint32_t n_runs, n_components;
} whamd_debug_head_plan_result;
whamd_status_t whamd_debug_head_first_plan(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                           const whamd_pedigree_view* pedigree, int distrust_genotypes,
                                           const uint32_t* positions, size_t n_positions, uint32_t head_pieces, whamd_debug_head_plan_result* out);

/* HOST-ONLY export of the genotyper's run plan (csrc/genotype_plan.h; no device needed): the runs of the run-fused path in table order, and for
 * each where its chains rescale.  rescale_f / rescale_b: the run divides the column that enters it, forward (from run - 1) / backward
 * (from run + 1), by that column's total -- the run starts from a scaled total of 1; nothing is rescaled inside a run.  The wiring
 * behind it: a rescaling run reads n_part_in_* per-workgroup partial sums from part_in_* on, which are the n_part_out sums its neighbour leaves at
 * part_out_* when its emit_* is set.  *min_total_out: the scaled column total below which a solve discards the run path's result and takes
 * the per-column kernels (GS_MIN_TOTAL).  With both, a test can work out from a reference's per-column normalisers how small the numbers
 * of the device get.  WHAMD_ERR_UNSUPPORTED: the table is not eligible for the run path.  At most `capacity` runs are written to out[]
 * (may be NULL), *n_out: how many there are. */
typedef struct whamd_debug_genotype_run {
	uint32_t c0, ncols;
	uint32_t rescale_f, rescale_b, emit_f, emit_b;
	uint32_t n_part_out, part_out_f, part_out_b;
	uint32_t part_in_f, n_part_in_f, part_in_b, n_part_in_b;
	uint32_t reserved;
} whamd_debug_genotype_run;
whamd_status_t whamd_debug_genotype_run_plan(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                             const whamd_pedigree_view* pedigree, const uint32_t* positions, size_t n_positions,
                                             whamd_debug_genotype_run* out, size_t capacity, size_t* n_out, double* min_total_out);

/* HOST-ONLY twins of the polyphase threading inputs (csrc/polythread.cpp): the same validation, then rows, selection and haplotypes on one
 * host thread through the functions the kernels call (csrc/polythread.h); bit-identical to the device. */
whamd_status_t whamd_debug_poly_thread_inputs_host(const whamd_poly_thread_view* problems, uint64_t n_problems, whamd_poly_thread_result** out);
whamd_status_t whamd_debug_poly_select_clusters_host(uint64_t n_pos, const uint64_t* pc_ptr, const uint32_t* pc_cluster, const uint32_t* pc_total, uint32_t ploidy,
                                                     uint32_t max_cluster_gap, uint64_t* cov_ptr_out, uint32_t* cluster_out, uint8_t* readded_out, uint32_t* rank_out);
whamd_status_t whamd_debug_poly_haplotypes_host(const uint32_t* paths, uint64_t n_pos, uint32_t ploidy, const uint64_t* pc_ptr, const uint32_t* pc_cluster,
                                                const int8_t* pc_consensus, int8_t* haplotypes_out);

/* HOST-ONLY twin of the polyphase threading DP (csrc/polythreader.cpp): the same validation and host work, then the plain walk over all
 * pairs of tuples of neighbouring columns on one host thread; bit-identical to the device: scores, paths, ambiguous. */
whamd_status_t whamd_debug_poly_threader_host(const whamd_poly_threader_view* problems, uint64_t n_problems, whamd_poly_threader_result** out);

#ifdef __cplusplus
}
#endif

#endif /* WHATSHAP_AMD_DEBUG_H */
