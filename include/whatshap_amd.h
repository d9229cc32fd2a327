/*
 * whatshap_amd.h -- C ABI of the MI355X-native wMEC / PedMEC solver.
 *
 * This is the drop-in boundary for the hot path of `whatshap phase`: the C++ class
 * PedigreeDPTable that whatshap/core.pyx:364-416 binds through whatshap/cpp.pxd:85-90
 *
 *     PedigreeDPTable(ReadSet*, vector[unsigned int] recombcost, Pedigree*, bool distrust_genotypes,
 *                     vector[unsigned int]* positions) except +
 *     void get_super_reads(vector[ReadSet*]*, vector[unsigned int]* transmission_vector) except +
 *     int  get_optimal_score() except +
 *     vector[bool]* get_optimal_partitioning()
 *
 * Every entry point below replaces one of those four members (cited per function).  The ABI uses
 * plain pointers and sizes only: a ReadSet is handed over as a CSR "view" of what
 * src/readset.h / src/read.h store, a Pedigree as a view of what src/pedigree.h stores.  No torch,
 * no C++ types, no ownership transfer: every input pointer is borrowed for the duration of the call
 * that takes it (the table copies what it needs, unlike the reference, which keeps ReadSet* /
 * Pedigree* and re-reads them in get_super_reads, src/pedigreedptable.h:80-86).
 *
 * Error model: functions that can fail return a whamd_status_t; the message a Python binding
 * should raise as RuntimeError (the reference's `except +` path) is returned by
 * whamd_last_error().  The two messages of the reference's hot path are reproduced verbatim:
 *   "Error: Mendelian conflict"                          (src/pedigreedptable.cpp:302)
 *   "ColumnIterator: reads in ReadSet are not sorted."   (src/columniterator.cpp:29)
 *
 * Device selection: one table lives on one HIP device (one process per GPU, or one worker
 * thread per device); independent tables never communicate (no RCCL on this path).
 */
#ifndef WHATSHAP_AMD_H
#define WHATSHAP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: whamd_plan_summary grew (n_yform_runs, n_fact_runs), whamd_solve_stats.group_tables / host_flatten_ms: a caller built against
 * version 1 must not be handed the larger structs -- bindings compare whamd_abi_version() with the header they were built from. */
#define WHAMD_ABI_VERSION 4

/* allele codes, identical to Entry::allele_t (src/entry.h:8) */
#define WHAMD_ALLELE_REF 0
#define WHAMD_ALLELE_ALT 1
#define WHAMD_ALLELE_BLANK 2
#define WHAMD_ALLELE_EQUAL_SCORES 3

/* genotype codes of the pedigree view: canonical index of a diploid bi-allelic genotype
 * (src/genotype.h:22-27: 0 -> 0/0, 1 -> 0/1, 2 -> 1/1); anything else (other ploidy, other
 * alleles, empty genotype) is WHAMD_GT_OTHER and is compatible with no allele assignment,
 * exactly as Genotype::operator!= on the 64-bit code behaves (src/genotype.cpp:148-150). */
#define WHAMD_GT_OTHER 255

typedef enum whamd_status_t {
	WHAMD_OK = 0,
	WHAMD_ERR_INVALID = 1,           /* malformed input (message says what) */
	WHAMD_ERR_MENDELIAN_CONFLICT = 2, /* "Error: Mendelian conflict" */
	WHAMD_ERR_UNSORTED = 3,          /* ColumnIterator sortedness errors */
	WHAMD_ERR_UNSUPPORTED = 4,       /* outside the limits of the device path (coverage > 23, ...) */
	WHAMD_ERR_DEVICE = 5,            /* HIP runtime error / no device / extension missing */
	WHAMD_ERR_OVERFLOW = 6,          /* costs could exceed 32 bits; reference behaviour undefined there */
	WHAMD_ERR_HOST = 7               /* a host-side failure inside the library: out of memory, no thread could be started (message says what) */
} whamd_status_t;

/* View of a ReadSet (src/readset.h:14-26, src/read.h:10-83).  Reads in ReadSet order; the
 * variants of read r are entries read_ptr[r] .. read_ptr[r+1]-1 of the three var_* arrays. */
typedef struct whamd_readset_view {
	uint32_t n_reads;
	const uint64_t* read_ptr;       /* [n_reads + 1] */
	const int32_t* var_position;    /* Read::getPosition   */
	const uint8_t* var_allele;      /* Read::getAllele (0 = REF, 1 = ALT) */
	const uint32_t* var_quality;    /* Read::getVariantQuality (phred) */
	const int32_t* read_sample_id;  /* [n_reads] Read::getSampleID (numeric sample id) */
} whamd_readset_view;

/* View of a Pedigree (src/pedigree.h:16-86).  Individuals in insertion order (that order is
 * the "individual index"); triples by numeric id as passed to Pedigree::addRelationship. */
typedef struct whamd_pedigree_view {
	uint32_t n_individuals;
	const uint32_t* individual_id; /* [n_individuals] */
	uint32_t n_triples;
	const uint32_t* triple_ids;    /* [3 * n_triples]: father id, mother id, child id */
	uint32_t n_variants;           /* Pedigree::get_variant_count() (0 if no individual) */
	const uint8_t* genotype;       /* [n_individuals * n_variants] WHAMD genotype codes */
	const double* genotype_likelihoods; /* [n_individuals * n_variants * 3] phred GL of 0/0, 0/1, 1/1, or NULL */
	const uint8_t* gl_present;     /* [n_individuals * n_variants] 1 if the GL triple is set, or NULL (= all set iff genotype_likelihoods != NULL) */
} whamd_pedigree_view;

typedef struct whamd_dptable whamd_dptable; /* opaque */

/* Per-solve measurements taken with HIP events on the table's own stream. */
typedef struct whamd_solve_stats {
	uint64_t n_columns;
	uint64_t n_cells;            /* sum_c 2^k_c (unique bipartitions) */
	uint64_t n_costs;            /* n_cells * T */
	uint64_t algorithmic_bytes;  /* sum_c 4*T*2^b_c + 12*T*2^f_c + 12*k_c   */
	uint64_t forward_launches;   /* launches of the dominant (column-step) kernel (a solve that continued behind the table's preview -- option "preview" -- counts the preview's too) */
	double forward_ms;           /* HIP-event time of the forward pass (all column steps).  A solve that continued behind the table's preview: ONE interval, from the event
	                              * in front of the preview's first launch (inside whamd_dptable_create) to the end of the forward pass -- it contains whatever time the device
	                              * idled between the preview's last launch and the caller's enqueue, so it grows if the caller delays the enqueue; total_ms likewise.  A
	                              * caller that reads these as kernel time passes "preview" = "0". */
	double backtrace_ms;         /* HIP-event time of the device backtrace */
	double total_ms;             /* HIP-event time forward + backtrace + path download */
	double host_prepare_ms;      /* wall: flattening + descriptor build + upload (outside total_ms) */
	double host_finish_ms;       /* wall: superreads + partitioning on the host */
	uint32_t max_coverage;       /* max_c k_c */
	uint32_t transmissions;      /* T = 4^triples */
	uint32_t bt_chunks;          /* chunked speculative backtrace: chunks walked at once (0: the sequential walk was used) */
	uint32_t bt_missed;          /*   chunks whose true entry state was none of the guesses */
	uint32_t bt_rewalked;        /*   units walked again from the true state */
	uint32_t group_tables;       /* tables that shared this solve's forward launches (whamd_dptable_enqueue_many groups tables of one device;
	                              * 1: the table ran alone).  forward_ms / forward_launches then describe the GROUP's launches. */
	double host_flatten_ms;      /* the part of host_prepare_ms spent flattening the ReadSet (ColumnIterator's work, src/columniterator.cpp:91-169):
	                              * host_prepare_ms - host_flatten_ms = indexing scheme, cost terms, plan and upload -- what the reference's constructor
	                              * does before compute_table (src/pedigreedptable.cpp:15-37; SURVEY.md 8d puts it inside the solve time) */
} whamd_solve_stats;

/* Library / device introspection. */
int whamd_abi_version(void);
/* number of visible HIP devices (0 if none; never fails) */
int whamd_device_count(void);
/* PCI bus id of HIP device `device` ("0000:c5:00.0") into `out` (at most `capacity` bytes incl. the terminator): what a launcher needs to find
 * the NUMA node / CPU list of the device in sysfs (/sys/bus/pci/devices/<id>/numa_node, local_cpulist) and keep rank r's host threads next
 * to GPU r (whatshap_amd.blocks.bind_rank_to_device_cpus).  No reference counterpart: the reference has no device.  WHAMD_ERR_DEVICE if
 * there is no such device, WHAMD_ERR_INVALID for a null / too small buffer. */
whamd_status_t whamd_device_pci_bus_id(int device, char* out, size_t capacity);
/* thread-local message of the last failing call on this thread ("" if none) */
const char* whamd_last_error(void);

/* Frees everything the table holds on the device (buffers, stream, events) while keeping the solution: the getters
 * below stay valid, a later enqueue/solve uploads again.  For callers that keep thousands of solved blocks alive
 * (one table per connected component of a chromosome).  No reference counterpart: the reference frees its
 * backtrace tables only in ~PedigreeDPTable (src/pedigreedptable.cpp:40-48). */
whamd_status_t whamd_dptable_release_device(whamd_dptable* table);

/* whamd_dptable_enqueue for several tables at once: their launch sequences are submitted round robin, a few launches
 * per table and turn, so that the streams of independent blocks fill up side by side and the blocks overlap on the
 * device from the first column on (submitting table after table lets each one run alone for as long as the host needs
 * to submit the next).  Collect every table with whamd_dptable_wait.  No reference counterpart (the reference solves
 * blocks one after the other, cli/phase.py:604). */
whamd_status_t whamd_dptable_enqueue_many(whamd_dptable* const* tables, size_t n_tables);
/* whamd_dptable_wait for several tables: every table's device side is collected, then the host side of all of them (superreads and
 * partitioning: what get_super_reads / get_optimal_partitioning compute, src/pedigreedptable.cpp:344-406) runs on a few host threads at
 * once.  Returns the first failure; every table has left the "in flight" state afterwards. */
whamd_status_t whamd_dptable_wait_many(whamd_dptable* const* tables, size_t n_tables);

/*
 * Replaces PedigreeDPTable::PedigreeDPTable (src/pedigreedptable.cpp:15-37), split in two so that
 * a benchmark can time the device part alone:
 *
 *   whamd_dptable_create : ColumnIterator construction + validation (src/columniterator.cpp:10-59),
 *                          ColumnIndexingScheme per column (src/columnindexingscheme.cpp:7-34,62-85),
 *                          PedigreePartitions (src/pedigreepartitions.cpp:7-42), allele-assignment
 *                          tables (src/pedigreecolumncostcomputer.cpp:14-50); uploads them to `device`.
 *   whamd_dptable_solve  : compute_table() (src/pedigreedptable.cpp:84-174) on the device:
 *                          forward pass over all columns, backtrace -> index path; then the host
 *                          part of get_super_reads / get_optimal_partitioning is evaluated once and
 *                          cached.  May be called repeatedly (re-solves from the uploaded input).
 *
 * recombcost has n_recombcost entries; the reference indexes recombcost[column] without a bounds
 * check (src/pedigreedptable.cpp:289) -- here a missing tail is padded with the last given value
 * (0 if empty).  positions == NULL means ReadSet::get_positions() (src/readset.cpp:54-62).
 * Does NOT mutate the caller's ReadSet (the reference's reassignReadIds(), :24, has no
 * counterpart on a view).
 */
whamd_status_t whamd_dptable_create(const whamd_readset_view* readset, const uint32_t* recombcost,
                                    size_t n_recombcost, const whamd_pedigree_view* pedigree,
                                    int distrust_genotypes, const uint32_t* positions, size_t n_positions,
                                    int device, whamd_dptable** out);
/* whamd_dptable_create -- the replacement of PedigreeDPTable::PedigreeDPTable (src/pedigreedptable.cpp:15-37, see above) -- with solver
 * options (the keys of whamd_dptable_set_option) applied BEFORE the plan is made and uploaded: one upload instead of two.  What it is for: tables that will share their launches with many others (whamd_dptable_enqueue_many) do
 * better with eight cells per thread and twelve local slots when they are wide: "shared_launches" = "1" says so (the library applies the
 * layout to single-individual tables of coverage >= 18: half the wavefronts per table, 24 coverage-20 tables 7.7 M columns/s instead of
 * 6.4 M), while a table solved alone is faster with the default four cells (2.26 M against 1.87 M) and narrow tables gain nothing.
 * "host_threads" = "n" (this call only): how many host threads the create may use -- a caller that creates many tables on threads of its
 * own keeps each to a few. */
whamd_status_t whamd_dptable_create_with_options(const whamd_readset_view* readset, const uint32_t* recombcost,
                                                 size_t n_recombcost, const whamd_pedigree_view* pedigree,
                                                 int distrust_genotypes, const uint32_t* positions, size_t n_positions,
                                                 const char* const* keys, const char* const* values, size_t n_options,
                                                 int device, whamd_dptable** table_out);
whamd_status_t whamd_dptable_solve(whamd_dptable* table);
/* The two halves of whamd_dptable_solve, for the host-side work queue: _enqueue submits the table's launches to its
 * own HIP stream and returns; _wait blocks until the index path has arrived and evaluates the host part.  Several
 * tables (independent phasing blocks) may be in flight on one device at once -- their kernels overlap. */
whamd_status_t whamd_dptable_enqueue(whamd_dptable* table);
whamd_status_t whamd_dptable_wait(whamd_dptable* table);
/* ~PedigreeDPTable (src/pedigreedptable.cpp:40-46) */
void whamd_dptable_destroy(whamd_dptable* table);

/* Shape queries (valid after create). */
uint64_t whamd_dptable_column_count(const whamd_dptable* table);     /* ColumnIterator::get_column_count */
uint32_t whamd_dptable_individual_count(const whamd_dptable* table); /* Pedigree::size */
uint32_t whamd_dptable_read_count(const whamd_dptable* table);       /* ReadSet::size */
/* positions[column_count]: ColumnIterator::get_positions (src/columniterator.cpp:81-83) */
whamd_status_t whamd_dptable_positions(const whamd_dptable* table, uint32_t* positions_out);

/* PedigreeDPTable::get_optimal_score (src/pedigreedptable.cpp:338-341). Valid after solve. */
whamd_status_t whamd_dptable_get_optimal_score(const whamd_dptable* table, uint32_t* score_out);

/*
 * PedigreeDPTable::get_super_reads (src/pedigreedptable.cpp:344-388).  Instead of building Read
 * objects the ABI returns their contents; the binding creates, per individual i (pedigree order),
 * Read("superread_0_<i>", -1, -1, sample_id_out[i]) and Read("superread_1_<i>", ...) and adds, for
 * column c, (positions[c], allele0_out[i*n + c], quality_out[i*n + c]) resp. allele1_out.
 *   allele*_out  : [n_individuals * n_columns], values 0, 1 or 3 (EQUAL_SCORES)
 *   quality_out  : [n_individuals * n_columns]
 *   transmission_out : [n_columns]  (index_path[c].inheritance_value)
 *   sample_id_out    : [n_individuals] (Pedigree::index_to_id)
 * Any output pointer may be NULL to skip it.
 */
whamd_status_t whamd_dptable_get_super_reads(const whamd_dptable* table, uint8_t* allele0_out,
                                             uint8_t* allele1_out, uint32_t* quality_out,
                                             uint32_t* transmission_out, uint32_t* sample_id_out);

/* PedigreeDPTable::get_optimal_partitioning (src/pedigreedptable.cpp:391-406) with the Cython
 * post-processing of core.pyx:413-416 already applied: partition_out[r] in {0, 1} is the side
 * (the bit) of read r; reads never active get 1. */
whamd_status_t whamd_dptable_get_optimal_partitioning(const whamd_dptable* table, uint8_t* partition_out);

/* The raw backtrace result (index_path, src/pedigreedptable.h:17-21,54): bipartition index and
 * transmission value per column.  Not exposed by the reference's Cython layer; used by parity tests. */
whamd_status_t whamd_dptable_get_index_path(const whamd_dptable* table, uint32_t* index_out,
                                            uint32_t* transmission_out);

/* Measurements of the last whamd_dptable_solve on this table. */
whamd_status_t whamd_dptable_get_stats(const whamd_dptable* table, whamd_solve_stats* stats_out);

/* Options (for A/B measurements and tests), effective at the next solve:
 *   "path"          "auto" (default: slot runs for a single individual and for one or two trios -- pedigree slot runs, csrc/kernels_pedslots.h --,
 *                   the per-column kernels for larger pedigrees) | "slots" | "resident" (round 1's LDS-resident runs, kept for comparison) |
 *                   "column" (one launch per column, the general path) | "column_keys"
 *   "slot_l"        preferred number of local slots of a slot run (slot_r + 6 .. slot_r + 9: 1 .. 8 waves per workgroup)
 *   "slot_r"        reg slots of a slot run: "2" (4 cells per thread, default) or "3" (8 cells per thread)
 *   "arena_limit_bytes"  upper bound of the backtrace arena (default: what free HBM allows).  A table whose records need
 *                   more is solved in windows: the forward pass keeps the projection column at every window boundary and
 *                   the steps of every window but the newest are run a second time right before their records are walked
 *                   (same result, up to twice the forward time, any table length).
 *   "resident_l"    preferred log2 slice size of the run kernels
 *   "resident_fold" "0" disables folding of columns without an ending read
 *   "symmetry"      single individual: D[~x] == D[x], so a run may compute half of its workgroups only: "0" never,
 *                   "1" runs that would fill the chip (default), "2" every run with a grid read (tests)
 *   "lanes"         how many connected components of a single-individual table advance side by side (default 32, their
 *                   runs go out as batched launches; "1" solves them one after the other)
 *   "preview"       "auto" (default) | "0" | "1".  whamd_dptable_create of a single-individual table on slot runs may launch the table's leading
 *                   runs itself, right behind the plan and from a small upload of their own, so that the device works while the rest of the table
 *                   is built and uploaded; the first whamd_dptable_enqueue of the table, alone on its own stream and with no option changed since,
 *                   continues behind them.  The finished schedule is compared with what was launched, run by run; where anything differs, and in
 *                   every other case (whamd_dptable_enqueue_many with other tables, a second solve, an option set after the create), the solve
 *                   starts at its first step as ever: the result never depends on the preview.  "auto": only a table of eight plan pieces (about
 *                   65 000 columns) and more, one connected component, created without "host_threads" and "shared_launches" while no other
 *                   table of the process holds resources on the device -- a caller with many tables in flight gains nothing from it.  "1": every
 *                   table whose form allows it (tests).  Give it with whamd_dptable_create_with_options: the create is where it acts.
 *   "preview_pieces"  how many plan pieces (of about 8 192 columns) the preview covers; "0" (default): a sixth of the table's. */
whamd_status_t whamd_dptable_set_option(whamd_dptable* table, const char* key, const char* value);

/*
 * Host-only diagnostics (no device needed): builds the flattened problem and the forward plan exactly as
 * whamd_dptable_create would and reports how the columns are scheduled.  Used by the CPU test-suite to check
 * the planner's invariants (every column in exactly one step, runs within the LDS budget, ...).
 */
typedef struct whamd_plan_summary {   /* (the CPU plan emulators that used to be declared below live in whatshap_amd_debug.h: test-only library) */
	uint64_t n_columns;
	uint64_t n_steps;             /* launches of the forward pass (runs + per-column steps) */
	uint64_t n_runs;              /* resident runs (one launch each) */
	uint64_t n_resident_columns;  /* columns executed inside runs */
	uint64_t n_folded_columns;    /* resident columns evaluated inside their successor (no barrier of their own) */
	uint64_t n_vectorised_columns;/* resident columns on the 4-entries-per-thread path (incl. folded) */
	uint64_t max_run_columns;
	uint64_t max_workgroups;      /* largest grid of a run */
	uint64_t max_lds_bytes;       /* largest dynamic LDS request of a run */
	uint64_t backtrace_bytes;     /* size of the backtrace arena */
	uint64_t n_components;        /* connected components the device driver may run as independent jobs (single individual) */
	uint64_t n_halved_runs;       /* runs that launch only half of their workgroups (complement symmetry) */
	uint32_t max_coverage;
	uint32_t invariants_ok;       /* 1 if the internal consistency checks passed */
	uint64_t n_yform_runs;        /* slot runs that compute in Y form (one absolute difference per cell-column; slots.h) */
	uint64_t n_fact_runs;         /* pedigree slot runs on factorised lines (a trio or a quartet whose genotypes are not trusted; slots.h PSLOT_FACT, PSLOT_FACT4) */
} whamd_plan_summary;
whamd_status_t whamd_plan_summarize(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                    const whamd_pedigree_view* pedigree, int distrust_genotypes,
                                    const uint32_t* positions, size_t n_positions, const char* path,
                                    whamd_plan_summary* out);

/* ---- PedMecHeuristic: the beam-search sibling of PedigreeDPTable behind the same Python API -------------
 * Replaces cpp.PedMecHeuristic (whatshap/cpp.pxd:260-268; src/pedmecheuristic.h:56-120): constructor arguments of
 * whatshap/core.pyx:674-689 (row_limit, allow_mutations; verbosity has no counterpart), solve() is part of _create as the
 * wrapper's getters all call it first (core.pyx:695).  The ReadSet must be sorted (whatshap/cli/phase.py:590 sorts it) and
 * the pedigree's individuals must carry the ids 0 .. n-1 in insertion order (the reference mixes ids, indices and ranks,
 * src/pedmecheuristic.cpp:49-82).  One persistent workgroup per table (csrc/heuristic_device.hip), any number of tables per launch
 * (whamd_pedmec_heuristic_enqueue_many); every decision of the beam equals the reference's (float scores restated operation by operation). */
typedef struct whamd_heuristic whamd_heuristic; /* opaque */
typedef struct whamd_heuristic_stats {
	uint64_t n_columns, n_reads;
	uint64_t max_solutions;      /* widest column of the beam */
	uint64_t total_solutions;    /* sum over the columns */
	double device_ms;            /* HIP events around the kernel */
	double host_prepare_ms;      /* flattening + per-column bookkeeping + upload (wall) */
	double host_finish_ms;       /* allele votes + phasing per column (wall) */
	uint32_t n_samples, row_limit;
} whamd_heuristic_stats;
whamd_status_t whamd_pedmec_heuristic_create(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                             const whamd_pedigree_view* pedigree, int distrust_genotypes,
                                             const uint32_t* positions, size_t n_positions, uint32_t row_limit, int allow_mutations,
                                             int device, whamd_heuristic** out);
/* Several tables at once, asynchronously: every job is what whamd_pedmec_heuristic_create takes.  _enqueue_many builds the plans (a few
 * host threads), uploads them and submits ONE launch whose grid is the tables -- one persistent workgroup each, on a stream of the batch's
 * own -- and returns with out[i] in flight; whamd_pedmec_heuristic_wait(out[i]) collects (the first wait on any handle of a batch collects
 * the whole batch; the getters fail on a handle still in flight).  Independent tables are what `whatshap phase --algorithm heuristic`
 * produces per chromosome x family (whatshap/cli/phase.py:467,486,589-603).  The input arrays are only read during _enqueue_many. */
typedef struct whamd_heuristic_job {
	const whamd_readset_view* readset;
	const uint32_t* recombcost;
	size_t n_recombcost;
	const whamd_pedigree_view* pedigree;
	int distrust_genotypes;
	const uint32_t* positions;
	size_t n_positions;
	uint32_t row_limit;
	int allow_mutations;
} whamd_heuristic_job;
whamd_status_t whamd_pedmec_heuristic_enqueue_many(const whamd_heuristic_job* jobs, size_t n_jobs, int device, whamd_heuristic** out);
whamd_status_t whamd_pedmec_heuristic_wait(whamd_heuristic* h);
uint64_t whamd_pedmec_heuristic_column_count(const whamd_heuristic* h);
uint32_t whamd_pedmec_heuristic_sample_count(const whamd_heuristic* h);
uint32_t whamd_pedmec_heuristic_read_count(const whamd_heuristic* h);
/* score: getOptScore (the reference never assigns it: 0); bipartition[reads]: getOptBipartition bits; transmission[columns]:
 * getOptTransmission; haplotypes / mutated [samples][2][columns]: getOptHaplotypes / getMutations; sample_ids[samples]: the
 * global ids getSuperReads gives its reads; positions[columns].  NULL pointers are skipped. */
whamd_status_t whamd_pedmec_heuristic_get(const whamd_heuristic* h, float* score, uint8_t* bipartition, uint32_t* transmission,
                                          int8_t* haplotypes, uint8_t* mutated, uint32_t* sample_ids, uint32_t* positions);
whamd_status_t whamd_pedmec_heuristic_get_stats(const whamd_heuristic* h, whamd_heuristic_stats* stats_out);
void whamd_pedmec_heuristic_destroy(whamd_heuristic* h);

/* The tie-break hash of ReadSet::sort (src/readset.h:39-66,76-82): std::hash<std::string>(name) ^
 * std::hash<int>(source_id) of the libstdc++ this library is built against.  Used by the Python
 * mirror of ReadSet.sort(); not part of the DP path. */
uint64_t whamd_read_sort_hash(const char* name, int source_id);

/* Read selection (whatshap/readselect.pyx:218-255 readselection(readset, max_cov, preferred_source_ids, bridging)):
 * selected_out[r] = 1 for every read the reference would return, 0 otherwise.  Host code (a priority queue; SURVEY.md
 * section 8 row f2); ties are resolved as the reference resolves them under CPython 3.10 / libstdc++ (readselect.cpp).
 * read_source_id: [n_reads] Read::getSourceID, may be NULL when n_preferred == 0.  A read with fewer than two variants
 * is WHAMD_ERR_INVALID (the reference raises ValueError).  Uses var_position and var_quality of the view. */
whamd_status_t whamd_readselection(const whamd_readset_view* readset, const int32_t* read_source_id,
                                   const int32_t* preferred_source_ids, size_t n_preferred, uint32_t max_cov, int bridging,
                                   uint8_t* selected_out, uint64_t* n_selected);

/* ---- GenotypeDPTable -----------------------------------------------------------------
 * Replaces  cppclass GenotypeDPTable (whatshap/cpp.pxd:118-121; src/genotypedptable.cpp):
 *     GenotypeDPTable(ReadSet*, vector[unsigned int] recombcost, Pedigree* pedigree, vector[unsigned int]* positions)
 *     vector[long double] get_genotype_likelihoods(unsigned int individual_id, unsigned int position)
 * One call = constructor (the whole forward-backward pass) + get_genotype_likelihoods for every individual and column.
 * The pedigree view must carry genotype_likelihoods: here they are the genotype PRIORS (probabilities of 0/0, 0/1, 1/1;
 * the reference asserts they are present, src/transitionprobabilitycomputer.cpp:66); its `genotype` codes are not used.
 * gl_out: [n_individuals][n_columns][3], every triple sums to 1.  n_columns = n_positions, or the number of distinct
 * read positions when positions is NULL; gl_capacity (in doubles) must be at least n_individuals * n_columns * 3.
 * Arithmetic is f64 (the reference: long double): results agree to a relative tolerance (~1e-12), not bit for bit. */
typedef struct whamd_genotype_stats {
	uint64_t n_columns;
	uint64_t n_cells;        /* sum_c 2^k_c */
	uint64_t launches;
	double backward_ms;      /* HIP events: backward pass that leaves the kept columns */
	double forward_ms;       /* HIP events: windows (backward recompute + forward + normalisation) */
	double total_ms;
	double host_prepare_ms;  /* wall: flattening + model tables + upload + solve + download, minus total_ms */
	uint32_t window;         /* columns per window */
	uint32_t max_coverage;
	uint32_t transmissions;
	uint32_t slot_runs;      /* launches per chain of the run-fused path (genotype_slots.hip); 0: the per-column kernels ran */
} whamd_genotype_stats;
whamd_status_t whamd_genotype_likelihoods(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                          const whamd_pedigree_view* pedigree, const uint32_t* positions, size_t n_positions,
                                          int device, uint32_t window, double* gl_out, size_t gl_capacity,
                                          whamd_genotype_stats* stats_out);

/* Everything the library keeps between calls goes back to the driver: the column store of whamd_genotype_likelihoods (tens of GB for long
 * inputs, one block per device: mapping that much fresh device memory takes seconds), the backtrace arena of the table closed last
 * (commonly > 10 GB), the pinned upload staging area of whamd_dptable_create (up to 1 GiB of host memory) and the device buffers of
 * the PedMecHeuristic solves.  Blocks in use are not touched. */
void whamd_release_caches(void);
/* Host memory the library keeps idle between tables, in bytes: a table's large arrays (columns, entries, plan rows, descriptors, solution -- 45 MB for a
 * coverage-15 table of 50 000 columns, 200 MB for configs[2]) go back to a process-wide pool when the table is destroyed and are reused by the next create
 * (csrc/host_memory.cpp: freeing and re-faulting them was 6 ms per configs[2] table and 0.7 ms per small one, and serialised concurrent creates).
 * whamd_release_caches() returns them to the system; WHAMD_HOST_POOL_MB bounds the pool (default 16384, 0 switches it off).  No reference counterpart:
 * the reference frees everything with the table. */
uint64_t whamd_host_pool_idle_bytes(void);

/* ---- Allele detection by re-alignment (ReadSetReader.detect_alleles_by_alignment, whatshap/variants.py:685-912) ----------------
 * For every (alignment, variant) pair that _iterate_cigar (whatshap/_variants.pyx:10-81) yields, ReadSetReader.realign cuts a window of
 * the read, builds one padded window per allele and keeps the allele whose edit distance to the read window is strictly smallest
 * (unit costs: edit_distance, quality 30; affine: edit_distance_affine_gap, quality d0 - d1, whatshap/align.pyx:16-196).  Here the
 * CIGAR walk and the windows are computed on the host (csrc/realign.cpp, several threads), the distances and the decision on the
 * device (csrc/realign_device.hip); only the per-job result comes back.  Views carry no pysam object; every pointer is borrowed for
 * the duration of the call.
 * Errors (WHAMD_ERR_INVALID, nothing launched) carry the reference's exception as a prefix of the message:
 *   "ValueError: Unsupported CIGAR operation: N"         (_iterate_cigar)
 *   "AssertionError: ..."                                (cigar_prefix_length, the window asserts of realign, unsorted variants,
 *                                                         affine costs without their parameters)
 *   "IndexError: list index out of range"                (an allowed allele set that keeps no allele)
 *   "TypeError: ..."                                     (a job on an alignment without query sequence)
 * When several alignments fail, the first one in alignment order is reported. */
typedef struct whamd_realign_alignments_view {
	uint64_t n_alignments;
	const int64_t* reference_start;  /* [n] AlignedSegment.reference_start */
	const uint64_t* first_variant;   /* [n] the `j` of detect_alleles_by_alignment, or NULL (0 for every alignment) */
	const uint64_t* cigar_ptr;       /* [n + 1] ops of alignment a: cigar_ptr[a] .. cigar_ptr[a+1]-1 */
	const uint32_t* cigar_op;        /* MIDNSHP=X as 0 .. 8 (anything else: ValueError when reached) */
	const uint32_t* cigar_len;
	const uint64_t* seq_ptr;         /* [n + 1] query_sequence bytes of alignment a: seq[seq_ptr[a] .. seq_ptr[a+1]-1] */
	const uint8_t* seq;
	const uint8_t* seq_present;      /* [n] 0: query_sequence is None; NULL: every alignment has one */
} whamd_realign_alignments_view;

typedef struct whamd_realign_variants_view {
	uint64_t n_variants;             /* in the order of the caller's list (the walk asserts what the reference asserts about it) */
	const int64_t* position;         /* [n] VcfVariant.position (0-based) */
	const uint64_t* ref_ptr;         /* [n + 1] reference_allele bytes */
	const uint8_t* ref_bytes;
	const uint64_t* alt_ptr;         /* [n + 1] alt alleles of variant v: alt_ptr[v] .. alt_ptr[v+1]-1 (allele index 1 ..) */
	const uint64_t* alt_byte_ptr;    /* [n_alts + 1] bytes of every alt allele */
	const uint8_t* alt_bytes;
	const uint64_t* restrict_ptr;    /* [n + 1] Genotype.as_vector() of restricted_genotypes[v], or NULL: no restriction at all */
	const int64_t* restrict_alleles;
	const uint8_t* restrict_present; /* [n] 0: no restriction for this variant; NULL: every variant has its list */
} whamd_realign_variants_view;

/* The reference as the bytes of one slice: bytes[k] is chromosome position offset + k.  chromosome_length is len(reference) (what
 * realign asserts against); the slice must cover every window (the span the alignments touch plus the overhang) or the call fails. */
typedef struct whamd_realign_reference_view {
	const uint8_t* bytes;
	uint64_t offset;
	uint64_t length;
	uint64_t chromosome_length;
} whamd_realign_reference_view;

/* overhang, use_affine, gap_start, gap_extend, default_mismatch of detect_alleles_by_alignment.  gap_start / gap_extend are what
 * the Cython int parameters hold (the binding truncates toward zero), default_mismatch is rounded to f32 as the float table is.
 * affine_unset = 1: use_affine with one of the three left as None -- the first job realign computes distances for fails with
 * "AssertionError: ..." where the reference asserts them (after slicing the query, before the distances); no job, no error. */
typedef struct whamd_realign_params {
	int64_t overhang;
	int32_t use_affine;
	int32_t gap_start;
	int32_t gap_extend;
	float default_mismatch;
	int32_t affine_unset;
} whamd_realign_params;

typedef struct whamd_realign_stats {
	uint64_t n_alignments;
	uint64_t n_jobs;                 /* (alignment, variant) pairs realign computed distances for (symbolic alleles make none) */
	uint64_t n_pairs;                /* (job, allele) distances */
	uint64_t n_results;              /* jobs with a decision (what the generator yields) */
	double host_walk_ms;             /* wall: CIGAR walk, windows, descriptors into the pinned staging buffer */
	double upload_ms;                /* HIP events: reference slice, variant tables, descriptors, query windows */
	double kernel_ms;                /* HIP events: distances + decision */
	double download_ms;              /* HIP events: the per-job results */
	double host_finish_ms;           /* wall: per-alignment result lists */
	double total_ms;                 /* wall of the whole call */
} whamd_realign_stats;

typedef struct whamd_realign whamd_realign; /* opaque */

/* One call for a batch of alignments against one variant list and one reference (a chromosome x sample of _alignments_to_reads). */
whamd_status_t whamd_realign_detect(const whamd_realign_alignments_view* alignments, const whamd_realign_variants_view* variants,
                                    const whamd_realign_reference_view* reference, const whamd_realign_params* params, int device,
                                    whamd_realign** out);
/* Results in the order detect_alleles_by_alignment yields them, alignment after alignment: (variant index, allele, quality) of
 * alignment a are entries ptr[a] .. ptr[a+1]-1.  ptr_out: [n_alignments + 1]; the others [whamd_realign_result_count].  NULL skips. */
uint64_t whamd_realign_result_count(const whamd_realign* r);
whamd_status_t whamd_realign_get(const whamd_realign* r, uint64_t* ptr_out, uint64_t* variant_out, int32_t* allele_out, int64_t* quality_out);
whamd_status_t whamd_realign_get_stats(const whamd_realign* r, whamd_realign_stats* stats_out);
void whamd_realign_destroy(whamd_realign* r);

/* Raw distances for a batch of (query, target) pairs: edit_distance(query, target) (unbanded, whatshap/align.pyx:16-97) or
 * edit_distance_affine_gap(query, target, mismatch_cost, gap_start, gap_extend) (:103-196) with one f32 mismatch cost per query
 * byte (mismatch_cost is laid out like `query`; NULL for unit costs).  distance_out: [n_pairs]. */
whamd_status_t whamd_edit_distance_batch(uint64_t n_pairs, const uint64_t* query_ptr, const uint8_t* query, const uint64_t* target_ptr,
                                         const uint8_t* target, int use_affine, const float* mismatch_cost, int32_t gap_start,
                                         int32_t gap_extend, int device, int64_t* distance_out);

/* ---- Polyphase read scoring (ReadScoring::scoreReadset, src/polyphase/readscoring.cpp:17-84) ----------------------------------------
 * For every pair of reads of an AlleleMatrix (src/polyphase/allelematrix.cpp:59-91) that share at least min_overlap positions, the sum
 * over the shared positions of log(P(same haplotype) / P(different haplotypes)), from genotype likelihoods of the allele depths.  Here
 * the matrix, the likelihoods (readscoring.cpp:123-191), the allele-pair tables (:193-225) and one float term per (position, allele,
 * allele) are computed on the host (csrc/polyscore.cpp); the pair loop runs on the device (csrc/polyscore_device.hip) and its results
 * are bit-identical to the host restatement of the debug library.  The reference sums the genotypes of a position in the iteration order
 * of an unordered_map; this library sums them in that order as GNU libstdc++ gives it (hash_order, csrc/polyscore.cpp).
 * A matrix is a CSR list of reads: read r lists (position, allele) entries read_ptr[r] .. read_ptr[r+1]-1, positions in genome
 * coordinates as Read::getPosition gives them, as AlleleMatrix(ReadSet*) takes them (:59-91): the first and last LISTED entry are the
 * read's first / last position, a position listed twice keeps the allele listed last and counts twice in the depths.  An empty read
 * has first position UINT32_MAX and last 0 (the readList constructor's convention, :45-47).
 * Errors (WHAMD_ERR_INVALID, nothing launched): a negative allele (undefined in the reference), an allele above 15 or a ploidy above 15
 * (Genotype's limits, src/genotype.h), a position outside [0, 2^32).  ploidy < 2 gives an empty result, as in the reference.
 * Results: per matrix, (i, j, score) with i > j in original read ids, sorted by the triangular index i*(i-1)/2 + j
 * (TriangleSparseMatrix::getIndices, trianglesparsematrix.cpp:66-73); scores that are exactly 0 are not stored, NaN scores are counted. */
typedef struct whamd_poly_matrix_view {
	uint64_t n_reads;
	const uint64_t* read_ptr;        /* [n_reads + 1] */
	const int64_t* position;         /* [read_ptr[n_reads]] */
	const int8_t* allele;            /* [read_ptr[n_reads]] */
} whamd_poly_matrix_view;

typedef struct whamd_poly_score_stats {
	double err;                      /* the allele error rate used: the caller's, or estimateAlleleErrorRate's when the caller passed 0 */
	uint64_t n_reads;
	uint64_t n_positions;
	uint64_t n_candidates;           /* pairs the reference's loop visits (readscoring.cpp:67-78; ties in first position by read id) */
	uint64_t n_overlapping;          /* candidate pairs that share at least min_overlap positions */
	uint64_t n_entries;              /* stored scores */
	uint64_t n_nan;                  /* NaN scores (counted, not stored: the reference's warning) */
	uint64_t n_pair_positions;       /* shared positions summed over the candidate pairs (the pair loop's table lookups) */
	uint32_t launches;               /* device steps of the whole call: pair loop, scan, compaction, sort (0: nothing touched the device) */
	double host_ms;                  /* wall, whole call: matrices, likelihoods, term tables, windows */
	double upload_ms;                /* HIP events, whole call */
	double kernel_ms;                /* HIP events, whole call: pair loop, compaction, sort */
	double download_ms;              /* HIP events, whole call */
	double total_ms;                 /* wall, whole call */
} whamd_poly_score_stats;

typedef struct whamd_poly_scores whamd_poly_scores; /* opaque: the result of one whamd_poly_score call */

/* One call for a batch of n_matrices matrices (polyphase scores one block at a time: small blocks share one launch sequence).  err == 0
 * estimates the error rate per matrix (readscoring.cpp:33-34). */
whamd_status_t whamd_poly_score(const whamd_poly_matrix_view* matrices, uint64_t n_matrices, uint32_t min_overlap, uint32_t ploidy, double err,
                                int device, whamd_poly_scores** out);
uint64_t whamd_poly_score_matrix_count(const whamd_poly_scores* s);
/* Entries of matrix m; i_out / j_out / score_out: [whamd_poly_score_count(s, m)], NULL skips. */
uint64_t whamd_poly_score_count(const whamd_poly_scores* s, uint64_t m);
whamd_status_t whamd_poly_score_get(const whamd_poly_scores* s, uint64_t m, uint32_t* i_out, uint32_t* j_out, float* score_out);
/* Counts and err of matrix m; the times are those of the whole call. */
whamd_status_t whamd_poly_score_get_stats(const whamd_poly_scores* s, uint64_t m, whamd_poly_score_stats* stats_out);
void whamd_poly_score_destroy(whamd_poly_scores* s);
/* ReadScoring::estimateAlleleErrorRate (readscoring.cpp:86-107): the err in 0.01, 0.02, ... (the reference's accumulating loop) whose
 * genotype likelihoods explain the depths best; host only, nothing printed. */
whamd_status_t whamd_poly_estimate_error_rate(const whamd_poly_matrix_view* matrix, uint32_t ploidy, double* err_out);

/* ---- Progeny marker scoring (get_variant_scoring, whatshap/polyphase/offspringscoring.py:143-188) ---------------------------------------
 * The "scoring" stage of polyphasegenetic: for every marker node i and every partner j = i + s of the stride list of scoring_window,
 * ProgenyGenotypeLikelihoods::get{SimplexNulliplex,SimplexSimplex,DuplexNulliplex}Score(i, j)
 * (src/polyphase/progenygenotypelikelihoods.cpp:116-149): log(1 / (ploidy - 1)) plus, over the progeny samples with data at both nodes in
 * increasing order, log(cooccur / disjoint) of two weighted sums of 4 or 6 likelihood products.  The host (csrc/progeny.cpp) finds the
 * stored entries and the row each of them reads; one device lane per entry walks the samples in double (csrc/progeny_device.hip).  Products
 * and sums are rounded one by one as the reference's are, so only log can differ from it (device math library against the host's).
 * The table is the reference's: float, [position][sample][genotype 0 .. ploidy], a sample without data at a position has a negative
 * genotype-0 value; a node at or beyond n_positions reads 0.0 everywhere (getGl, :72-76).  Only genotypes 0 .. 2 are read.
 * Stored entries, as the reference's loop stores them: -inf where both nodes belong to one variant; nothing for an anchor that is not
 * simplex-nulliplex (alt_count 1, co_alt_count 0); else the score kind follows the partner's variant type, (1, 0), (2, 0) or (1, 1) --
 * any other type is WHAMD_ERR_INVALID --, and a partner of the same variant as the partner scored before it stores that score again.
 * Errors (WHAMD_ERR_INVALID, nothing launched): ploidy < 2, scoring_window < 1 -- and scoring_window 1 .. 3, for which the reference's
 * stride list raises --, a node variant outside the type arrays, (n_positions + 1) * n_samples * (ploidy + 1) >= 2^32 (the reference's
 * uint32 index).  Results: per problem, (i, j) with i > j sorted by the triangular index i*(i-1)/2 + j, the double score and its float
 * rounding (TriangleSparseMatrix.set). */
typedef struct whamd_progeny_view {
	const float* gl;                 /* [n_positions][n_samples][ploidy + 1] */
	uint64_t n_positions;            /* numPositions of the reference's constructor */
	uint32_t n_samples;
	uint32_t ploidy;
	uint64_t n_nodes;                /* len(varinfo.get_node_positions()) */
	const uint32_t* node_variant;    /* [n_nodes] node_to_variant */
	uint64_t n_variants;
	const uint32_t* alt_count;       /* [n_variants] */
	const uint32_t* co_alt_count;    /* [n_variants] */
	uint32_t scoring_window;
} whamd_progeny_view;

typedef struct whamd_progeny_score_stats {
	uint64_t n_nodes;
	uint64_t n_entries;              /* stored entries */
	uint64_t n_inf;                  /* of them: set to -inf (both nodes of one variant) */
	uint64_t n_reused;               /* of them: the score of the partner before, stored again */
	uint64_t n_sample_terms;         /* (n_entries - n_inf) * n_samples: sample iterations of the pair loop */
	uint32_t launches;               /* kernel launches of the whole call (0: nothing touched the device) */
	double host_ms;                  /* wall, whole call: validation, entry lists */
	double upload_ms;                /* HIP events, whole call */
	double kernel_ms;                /* HIP events, whole call */
	double download_ms;              /* HIP events, whole call */
	double total_ms;                 /* wall, whole call (the repack of the tables included) */
} whamd_progeny_score_stats;

typedef struct whamd_progeny_scores whamd_progeny_scores; /* opaque: the result of one whamd_progeny_score call */

/* One call for a batch of problems (chromosomes, parents): one upload, one launch, one download. */
whamd_status_t whamd_progeny_score(const whamd_progeny_view* problems, uint64_t n_problems, int device, whamd_progeny_scores** out);
uint64_t whamd_progeny_score_problem_count(const whamd_progeny_scores* s);
/* Entries of problem m; the outputs are [whamd_progeny_score_count(s, m)], NULL skips. */
uint64_t whamd_progeny_score_count(const whamd_progeny_scores* s, uint64_t m);
whamd_status_t whamd_progeny_score_get(const whamd_progeny_scores* s, uint64_t m, uint32_t* i_out, uint32_t* j_out, float* score_f32_out,
                                       double* score_f64_out);
/* Counts of problem m; the times are those of the whole call. */
whamd_status_t whamd_progeny_score_get_stats(const whamd_progeny_scores* s, uint64_t m, whamd_progeny_score_stats* stats_out);
void whamd_progeny_score_destroy(whamd_progeny_scores* s);
/* get_most_likely_variant_type (offspringscoring.py:191-211) for n_nodes table rows (nodes == NULL: rows 0 .. n_nodes - 1): llh_out
 * [n_nodes][(ploidy+1)(ploidy+2)/2] holds the llh of every parental type (g0, g1 <= g0) in the reference's loop order, starting at 1.0 as
 * it does; g0_out / g1_out the first type with a strictly larger llh.  priors: [ploidy+1][ploidy+1][ploidy+1] (compute_gt_likelihood_priors).
 * One device lane per (row, type). */
whamd_status_t whamd_progeny_variant_types(const float* gl, uint64_t n_positions, uint32_t n_samples, uint32_t ploidy, const double* priors,
                                           const uint32_t* nodes, uint64_t n_nodes, int device, double* llh_out, uint32_t* g0_out, uint32_t* g1_out);

/* ---- Progeny genotype likelihoods (get_offspring_gl / compute_gt_likelihoods, whatshap/polyphase/offspringscoring.py:86-140, 232-274) ----
 * The table the two calls above read, made on the device from allele depths.  One cell is (depth row, sample) with ref_dp, alt_dp,
 * n = ref_dp + alt_dp: n < ploidy leaves all ploidy + 1 values at -1 (no data, the fill value of the reference's constructor); else
 * gl[g] = w_g / sum_g w_g, w_g = p_g^alt_dp * (1 - p_g)^ref_dp * prior[g] with p_g = (1 - g / ploidy) * error_rate + (g / ploidy) *
 * (1 - error_rate) formed in double as the reference forms it, prior = priors[row_alt_count][row_co_alt_count] (1 without priors), the sum
 * over g = 0 .. ploidy in that order, one division per value, rounded to float as setGlv stores it.  The binomial coefficient of the
 * reference's pmf cancels and is never formed; the powers are taken on (mantissa, exponent) pairs (csrc/progeny.h), so no depth a uint32
 * holds underflows or overflows; a weight 1000 binades or more below the largest counts 0.  Against the exact rational value of the doubles
 * p_g, 1.0 - p_g and prior[g]: |gl - exact| <= gamma(2n + ploidy + 1) * exact + 2^-999, gamma(m) = m 2^-53 / (1 - m 2^-53).
 * DIVERGENCE from the reference: where every pmf underflows it raises ZeroDivisionError or returns NaN (depths of a few hundred and more);
 * this returns the correctly normalised values.
 * A depth row is one progeny position under one (ref allele, alt allele, parental type); the nodes of one variant share it through
 * node_row.  One device lane per (sample, node) cell (progeny_gl_kernel, csrc/progeny_device.hip); host twin in the debug library.
 * Errors (WHAMD_ERR_INVALID, nothing launched): ploidy < 2, error_rate outside (0, 1), with priors a row_alt_count or row_co_alt_count
 * above the ploidy or a prior row that is negative, not finite or all zero, a node_row entry outside the rows,
 * (n_nodes + 1) * n_samples * (ploidy + 1) >= 2^32 (the reference's uint32 index, as whamd_progeny_score). */
typedef struct whamd_progeny_depths_view {
	const uint32_t* ref_depth;        /* [n_samples][n_rows]: allele_depths_of(sample)[progeny position][ref allele] */
	const uint32_t* alt_depth;        /* [n_samples][n_rows] */
	uint64_t n_rows;
	uint32_t n_samples;
	uint32_t ploidy;
	double error_rate;                /* allele_error_rate */
	const uint32_t* row_alt_count;    /* [n_rows] parental type of the row's first node (read with priors only) */
	const uint32_t* row_co_alt_count; /* [n_rows] */
	uint64_t n_nodes;                 /* rows of the table */
	const uint32_t* node_row;         /* [n_nodes] */
	const double* priors;             /* NULL: none, else [ploidy+1][ploidy+1][ploidy+1] (compute_gt_likelihood_priors) */
	/* whamd_progeny_score_depths only (as in whamd_progeny_view): */
	uint32_t scoring_window;
	const uint32_t* node_variant;     /* [n_nodes] */
	uint64_t n_variants;
	const uint32_t* alt_count;        /* [n_variants] */
	const uint32_t* co_alt_count;     /* [n_variants] */
} whamd_progeny_depths_view;

/* The tables of a batch of problems: one upload, one launch, one download.  table_out / table_f64_out: NULL, or [n_problems] pointers,
 * each NULL or the caller's array [n_nodes][n_samples][ploidy + 1] of problem m -- the float table, the doubles it was rounded from. */
whamd_status_t whamd_progeny_gl(const whamd_progeny_depths_view* problems, uint64_t n_problems, int device, float* const* table_out,
                                double* const* table_f64_out);
/* whamd_progeny_score on the tables of whamd_progeny_gl without either leaving the device: one upload (depths, entry lists), two launches
 * (progeny_gl_kernel writes the packed planes, progeny_pair_kernel reads them), one download.  Same result object, getters and stats. */
whamd_status_t whamd_progeny_score_depths(const whamd_progeny_depths_view* problems, uint64_t n_problems, int device, whamd_progeny_scores** out);

/* ---- Haplotagging (prepare_haplotag_information, whatshap/cli/haplotag.py:322-427) ------------------------------------------------------
 * The assignment step of `whatshap haplotag`: every read -- or group of linked reads -- goes to the phase set and the haplotype its alleles
 * support best.  One problem is one sample on one chromosome.  Strings stay with the caller: a read's representation (the key the
 * reference marks as processed) and its BX tag arrive as dense integer ids.
 * Grouping (host, in read order): a read whose representation was processed already is skipped; else it seeds a group, which, with
 * linked_reads != 0 and a BX tag, also takes every read of the same tag whose representation is not yet processed and whose start lies
 * within linked_read_cutoff of the seed's; all members are then processed.  Scoring (device, csrc/haplotag_device.hip): per phase set and
 * haplotype the sum (int64) of the qualities of the entries whose allele equals the haplotype's; a phase set exists for a group once one of
 * its entries matches a haplotype.  The winning phase set has the largest haplotype sum -- ties go to the one whose first matching entry
 * comes first, in the order seed, then the other members in read-set order, each read's variants as listed --; in it the best haplotype
 * is the lowest index among the maxima, quality = best - second best sum, and quality 0 leaves the group unassigned.  n_multiple_phase_sets
 * counts the groups with more than one phase set, assigned or not.
 * Errors (WHAMD_ERR_INVALID, nothing launched): ploidy outside 2 .. 16 (the reference raises IndexError at 1), an entry position that no
 * variant has (KeyError there), an entry allele outside {0, 1} (its assertion), variant positions that repeat. */
typedef struct whamd_haplotag_view {
	uint32_t ploidy;
	uint32_t linked_reads;              /* 0: --ignore-linked-read */
	int64_t linked_read_cutoff;
	uint64_t n_variants;
	const int64_t* variant_position;    /* [n_variants] distinct */
	const int64_t* variant_phaseset;    /* [n_variants] block_id */
	const int8_t* variant_phasing;      /* [n_variants][ploidy] haplotype alleles; a value other than 0 or 1 matches nothing */
	uint64_t n_reads;
	const uint64_t* read_ptr;           /* [n_reads + 1] into the entry arrays */
	const int64_t* entry_position;      /* [n_entries] */
	const int8_t* entry_allele;         /* [n_entries] */
	const int32_t* entry_quality;       /* [n_entries] */
	const int64_t* read_start;          /* [n_reads] reference_start */
	const uint32_t* read_repr;          /* [n_reads] dense id of the read's representation (equal ids: one representation) */
	const uint32_t* read_bx;            /* [n_reads] dense id of the BX tag, 0xffffffff: none; NULL: no read has one */
} whamd_haplotag_view;

typedef struct whamd_haplotag_stats {
	uint64_t n_reads;
	uint64_t n_groups;                  /* groups formed (reads skipped as processed form none) */
	uint64_t n_assigned;                /* groups that were assigned */
	uint64_t n_multiple_phase_sets;
	uint64_t n_entries;                 /* entries of all groups */
	uint64_t groups_class_a;            /* groups of 1 .. 64 entries: eight lanes each */
	uint64_t groups_class_b;            /* 65 .. 4096 entries: one wave each */
	uint64_t groups_class_c;            /* more: one workgroup each */
	uint64_t groups_many_phase_sets;    /* of them: more than 4 phase sets, one pass per phase set */
	uint32_t launches;                  /* kernel launches of the whole call (0: nothing touched the device) */
	double host_ms;                     /* wall, whole call: validation, grouping */
	double upload_ms;                   /* HIP events, whole call */
	double kernel_ms;                   /* HIP events, whole call */
	double download_ms;                 /* HIP events, whole call */
	double total_ms;                    /* wall, whole call */
} whamd_haplotag_stats;

typedef struct whamd_haplotag_result whamd_haplotag_result; /* opaque: the result of one whamd_haplotag call */

/* One call for a batch of problems (chromosomes x samples): one upload, at most three launches, one download. */
whamd_status_t whamd_haplotag(const whamd_haplotag_view* problems, uint64_t n_problems, int device, whamd_haplotag_result** out);
uint64_t whamd_haplotag_problem_count(const whamd_haplotag_result* r);
/* Reads of problem m. */
uint64_t whamd_haplotag_count(const whamd_haplotag_result* r, uint64_t m);
/* Per read of problem m: the haplotype (-1: the read's representation got no assignment from its group, or the read formed none), the
 * quality and the phase set; NULL skips. */
whamd_status_t whamd_haplotag_get(const whamd_haplotag_result* r, uint64_t m, int32_t* haplotype_out, int64_t* quality_out, int64_t* phaseset_out);
/* The assigned linked-read groups of problem m in processing order (what the reference appends to BX_tag_to_haplotype). */
uint64_t whamd_haplotag_bx_count(const whamd_haplotag_result* r, uint64_t m);
whamd_status_t whamd_haplotag_get_bx(const whamd_haplotag_result* r, uint64_t m, uint32_t* bx_out, int64_t* reference_start_out, int32_t* haplotype_out,
                                     int64_t* phaseset_out);
/* Counts of problem m; launches and times are those of the whole call. */
whamd_status_t whamd_haplotag_get_stats(const whamd_haplotag_result* r, uint64_t m, whamd_haplotag_stats* stats_out);
void whamd_haplotag_destroy(whamd_haplotag_result* r);

/* ---- Polyphase reordering (run_reordering without prephasing, whatshap/polyphase/reorder.py:139-194, 220-292, 351-407, 497-527) -----------
 * The third phase of `whatshap polyphase`: at every breakpoint of the threading, the log likelihood of each of the k! ways to link the k
 * affected haplotypes across it, the most likely linkage, and the threads and haplotypes permuted block by block accordingly.
 * One problem is one block: an AlleleMatrix (positions are its local indices 0 .. n_pos-1: n_pos must be the number of distinct positions
 * of the matrix), haplotypes[ploidy][n_pos] (any int8, -1 is a value like any other), threads[n_pos][ploidy], the clustering as CSR of read
 * ids, and per breakpoint its position in [1, n_pos), its sorted affected haplotypes (2 .. 8 of them) and the clusters whose reads are
 * collected, IN THE ORDER they are to be walked (the reference iterates a Python set of threads[pos][h] and threads[pos-1][h] over the
 * affected h; the Python wrapper evaluates the same expression).
 * Per breakpoint (host, csrc/polyreorder.cpp): the window -- up to 32 positions left of the breakpoint and up to 32 from it on at which
 * the affected haplotypes carry at least two values --; the reads of the listed clusters, in cluster order, with first < pos <= last
 * (getFirstPos / getLastPos of the matrix above), minus those extractSubMatrix(.., removeEmpty = true) drops: first >= the last window
 * position or last < the first (allelematrix.cpp:193; an empty window drops every read).
 * Device (csrc/polyreorder_device.hip): per kept read and affected haplotype, matches and errors left and right of the breakpoint over
 * the read's alleles at window positions, llh = log_match * (overlap - errors) + log_err * errors in double with every product and the
 * sum rounded on its own; per permutation, in lexicographic order, the sum over the reads IN ORDER, starting from +0.0, of the largest
 * left[affected[i]] + right[perm[i]].  log_match / log_err are the caller's log(1 - error_rate) / log(error_rate): the library calls no log.
 * Host again: per breakpoint the first largest llh in permutation order, the chained assignments (reorder.py:398-407), permute_blocks and
 * compute_breakpoint_confidence (host exp).
 * Errors (WHAMD_ERR_INVALID, nothing launched): what the matrix section lists; ploidy 0 or above 16; n_pos other than the matrix's
 * positions; an affected list unsorted, with repeats, shorter than 2, longer than 8 or naming a haplotype >= ploidy; a cluster or read
 * id out of range; breakpoint positions not strictly ascending or outside [1, n_pos). */
typedef struct whamd_poly_reorder_view {
	whamd_poly_matrix_view matrix;
	uint32_t ploidy;
	uint32_t reserved;                  /* 0 */
	uint64_t n_pos;
	const int8_t* haplotypes;           /* [ploidy][n_pos] */
	const int32_t* threads;             /* [n_pos][ploidy] */
	uint64_t n_clusters;
	const uint64_t* cluster_ptr;        /* [n_clusters + 1] into cluster_reads */
	const uint32_t* cluster_reads;      /* read ids of the matrix */
	uint64_t n_breakpoints;
	const uint64_t* bp_position;        /* [n_breakpoints] strictly ascending, in [1, n_pos) */
	const uint64_t* bp_affected_ptr;    /* [n_breakpoints + 1] into bp_affected */
	const uint32_t* bp_affected;        /* sorted haplotype indices */
	const uint64_t* bp_cluster_ptr;     /* [n_breakpoints + 1] into bp_clusters */
	const uint32_t* bp_clusters;        /* cluster ids in the order their reads are walked */
} whamd_poly_reorder_view;

typedef struct whamd_poly_reorder_stats {
	uint64_t n_breakpoints;
	uint64_t n_reads_visited;           /* kept reads summed over the breakpoints (rows of the left / right table) */
	uint64_t n_permutations;            /* k! summed over the breakpoints */
	uint64_t n_window_positions;        /* window positions summed over the breakpoints */
	uint32_t launches;                  /* kernel launches of the whole call: at most 2 (0: nothing touched the device) */
	double host_ms;                     /* wall, whole call: validation, matrices, windows, read lists */
	double upload_ms;                   /* HIP events, whole call */
	double kernel_ms;                   /* HIP events, whole call */
	double download_ms;                 /* HIP events, whole call */
	double total_ms;                    /* wall, whole call */
} whamd_poly_reorder_stats;

typedef struct whamd_poly_reorder_result whamd_poly_reorder_result; /* opaque: the result of one whamd_poly_reorder call */

/* One call for a batch of problems: one upload, at most two launches, one download. */
whamd_status_t whamd_poly_reorder(const whamd_poly_reorder_view* problems, uint64_t n_problems, double log_match, double log_err, int device,
                                  whamd_poly_reorder_result** out);
uint64_t whamd_poly_reorder_problem_count(const whamd_poly_reorder_result* r);
/* Breakpoints, llh values (k! summed over the breakpoints) and window positions of problem m. */
uint64_t whamd_poly_reorder_breakpoint_count(const whamd_poly_reorder_result* r, uint64_t m);
uint64_t whamd_poly_reorder_llh_count(const whamd_poly_reorder_result* r, uint64_t m);
uint64_t whamd_poly_reorder_window_count(const whamd_poly_reorder_result* r, uint64_t m);
/* llh_ptr_out: [breakpoints + 1] into llh_out; llh_out: per breakpoint its k! values in permutation order; best_out: [breakpoints] the
 * rank, in permutation order, of the first largest value; NULL skips. */
whamd_status_t whamd_poly_reorder_get_llh(const whamd_poly_reorder_result* r, uint64_t m, uint64_t* llh_ptr_out, double* llh_out, uint32_t* best_out);
/* window_ptr_out: [breakpoints + 1] into position_out; left_count_out: [breakpoints] how many of a breakpoint's positions lie left of it;
 * position_out: the window positions, ascending per breakpoint; NULL skips. */
whamd_status_t whamd_poly_reorder_get_windows(const whamd_poly_reorder_result* r, uint64_t m, uint64_t* window_ptr_out, uint32_t* left_count_out,
                                              uint32_t* position_out);
/* assignments_out: [breakpoints + 1][ploidy] (get_optimal_assignments); threads_out: [n_pos][ploidy] and haplotypes_out: [ploidy][n_pos]
 * after permute_blocks; confidence_out: [breakpoints]; NULL skips. */
whamd_status_t whamd_poly_reorder_get_phasing(const whamd_poly_reorder_result* r, uint64_t m, uint32_t* assignments_out, int32_t* threads_out,
                                              int8_t* haplotypes_out, double* confidence_out);
/* Counts of problem m; launches and times are those of the whole call. */
whamd_status_t whamd_poly_reorder_get_stats(const whamd_poly_reorder_result* r, uint64_t m, whamd_poly_reorder_stats* stats_out);
void whamd_poly_reorder_destroy(whamd_poly_reorder_result* r);

/* ---- Comparing polyploid phasings (`whatshap compare` above ploidy 2: compare_block, compute_switch_errors_poly and
 * compute_switch_flips_poly of whatshap/cli/compare.py on SwitchFlipCalculator::compare, src/polyphase/switchflipcalculator.cpp) -----------
 * One job is two phasings of the same positions, phasing0 and phasing1 as [n_pos][ploidy] alleles, and two costs.  The program is a
 * Viterbi pass over the ploidy! permutations of the haplotypes per visited position: a state costs flip_cost times the number of i with
 * phasing0[perm[i]] != phasing1[i], a transition switch_cost times the places in which two permutations differ.  matched_only visits
 * only the positions at which the two columns hold the same multiset of alleles (compute_matching_genotype_pos) and skips the rest.
 * States are ranked in the order of std::next_permutation from the identity (itertools.permutations(range(ploidy))).
 *
 * Identical to the reference: the total cost; the minimum Hamming distance; the matching positions; the switch-error count (flip cost
 * 2 * num_vars * ploidy + 1: no flip is chosen and the count is unique); the result for ONE visited position, switches = ploidy - 1 (the
 * reference's backtrace start counts the differences to Permutation::INVALID without a guard for position 0).
 * Defined here, because the reference's answer is an artefact of hash order (among equal candidates it takes the first in the iteration
 * order of a std::unordered_map): among the paths of minimum total cost the one with the fewest flips; among those, the predecessor of
 * lowest rank at every step and the end state of lowest rank.  Under this rule switches and flips depend on the input alone.  The
 * reference never has fewer flips.
 * Scores: min over q (score[q] + switch_cost * d) first, + flip_cost * f after, column 0 flip_cost * f alone, every product and sum
 * rounded on its own in double.
 * Device (csrc/polycompare_device.hip): one workgroup per job, one launch per call whatever the batch size (at most two are allowed
 * for).  Jobs with n_pos == 0 and matched_only jobs without a matching position return zeros; a call of only such jobs launches nothing.
 * Errors, all with nothing launched.  WHAMD_ERR_INVALID: ploidy below 2; a cost that is negative, NaN or infinite; a null array with
 * n_pos > 0.  WHAMD_ERR_UNSUPPORTED: ploidy above 6 (7! states are 25 M candidates per column; the reference itself warns above 6);
 * more than 2^28 positions in one job; want_path tables, n_visited * ploidy! * 2 bytes each, above WHAMD_POLY_COMPARE_MAX_PATH_BYTES in
 * total per call -- a limit, not a tuned number. */
#define WHAMD_POLY_COMPARE_MAX_PATH_BYTES ((uint64_t)1 << 30)

typedef struct whamd_poly_compare_view {
	uint32_t ploidy;
	uint32_t matched_only;              /* 0 / 1 */
	uint64_t n_pos;
	const uint8_t* phasing0;            /* [n_pos][ploidy] */
	const uint8_t* phasing1;            /* [n_pos][ploidy] */
	double switch_cost;
	double flip_cost;
	uint32_t want_path;                 /* 0 / 1: keep the state of every visited position */
	uint32_t reserved;                  /* 0 */
} whamd_poly_compare_view;

typedef struct whamd_poly_compare_job_result {
	double total;                       /* the minimum of the program: switch_cost * switches + flip_cost * flips of the chosen path */
	uint64_t n_matched;                 /* positions whose two allele multisets are equal (counted for every job) */
	uint64_t n_visited;                 /* n_matched with matched_only, else n_pos */
	uint64_t min_hamming_sum;           /* min over permutations of the disagreements summed over the visited positions */
	uint32_t switches;                  /* raw: not divided by ploidy */
	uint32_t flips;
} whamd_poly_compare_job_result;

typedef struct whamd_poly_compare_stats {
	uint64_t n_jobs;
	uint64_t n_positions;               /* summed over the jobs */
	uint64_t n_visited;                 /* positions visited, summed over the jobs */
	uint64_t path_bytes;                /* predecessor tables of the want_path jobs */
	uint32_t launches;                  /* kernel launches of the whole call: at most 2 (0: nothing touched the device) */
	double host_ms;                     /* wall: validation, matching positions */
	double upload_ms;                   /* HIP events */
	double kernel_ms;                   /* HIP events */
	double download_ms;                 /* HIP events */
	double total_ms;                    /* wall, whole call */
} whamd_poly_compare_stats;

typedef struct whamd_poly_compare_result whamd_poly_compare_result; /* opaque: the result of one whamd_poly_compare call */

/* One call for a batch of jobs: one upload, at most two launches, one download. */
whamd_status_t whamd_poly_compare(const whamd_poly_compare_view* jobs, uint64_t n_jobs, int device, whamd_poly_compare_result** out);
uint64_t whamd_poly_compare_job_count(const whamd_poly_compare_result* r);
/* Visited positions of job j that carry a path entry (0 without want_path). */
uint64_t whamd_poly_compare_path_count(const whamd_poly_compare_result* r, uint64_t j);
/* results_out: [jobs]. */
whamd_status_t whamd_poly_compare_get(const whamd_poly_compare_result* r, whamd_poly_compare_job_result* results_out);
/* Per visited position of job j, front to back like the reference's three lists after its reverse: position_out the position's index in
 * the job; rank_out the state's rank; perm_out [..][ploidy] the permutation; flipped_out [..][ploidy] 1 where phasing0[perm[i]] !=
 * phasing1[i]; switches_out the places in which the permutation differs from the previous position's (first position: 0, or ploidy - 1
 * when it is the only one).  NULL skips. */
whamd_status_t whamd_poly_compare_get_path(const whamd_poly_compare_result* r, uint64_t j, uint64_t* position_out, uint16_t* rank_out, uint8_t* perm_out,
                                           uint8_t* flipped_out, uint32_t* switches_out);
whamd_status_t whamd_poly_compare_get_stats(const whamd_poly_compare_result* r, whamd_poly_compare_stats* stats_out);
void whamd_poly_compare_destroy(whamd_poly_compare_result* r);

/* ---- Haplotagphase votes and consensus (compute_votes, consensus, best_candidate of whatshap/cli/haplotagphase.py:347-395, 203-304) -----------
 * `whatshap haplotagphase` phases the variants that are still unphased from reads that carry a phase set and a haplotype already.  One
 * problem is one sample on one chromosome: per variant a flag byte, the reads as CSR of (variant index, id, quality) -- id the index, 0 or
 * 1, of the read's allele in the sample's genotype vector at that variant -- and per read its phase set and haplotype, both reduced by 1
 * as the reference does (PS_tag - 1, HP_tag - 1).
 * Votes: a read with hp < 0 or ps < 0 is ignored; else one with hp > 1 is ignored and counted in n_skipped; every entry of any other read
 * whose variant is not homozygous adds its quality (int64 sums) to votes[variant][(ps, hp ^ id)].  Choice, per voted variant: the key with
 * the largest sum, ties to the phase set whose first voting entry at the variant comes first in the problem, within a phase set to
 * haplotype 0; score = that sum, total = all sums of the variant.  total == 0 sets zero_total (ZeroDivisionError there) and keeps nothing.
 * Filters, only where the variant is not phased: dropped if 100 * ((double)score / (double)total) < gap_threshold, or if only_indels and
 * the variant is an SNV.  (The reference's homopolymer filter can drop nothing -- its length is capped at the threshold it must exceed --
 * so no reference sequence is part of a problem.)
 * Device (csrc/tagphase_device.hip): count per variant, scan, place every voting entry into its variant's run, one team per variant
 * reduces and decides: 7 launches per call whatever the problems, 11 with a table; a call in which no entry votes launches nothing.
 * Errors, all with nothing launched.  WHAMD_ERR_INVALID: a null array, read_ptr that decreases or does not start at 0, a variant index
 * out of range, an id outside {0, 1}, flag bits above bit 2, a gap_threshold that is NaN.  WHAMD_ERR_UNSUPPORTED: the |quality| of a
 * problem's voting entries sum to more than 2^53 (beyond it the fraction would no longer be Python's: never answered approximately);
 * 2^32 - 1 or more variants or entries in one call; 2^30 or more phase sets in one problem. */
#define WHAMD_TAGPHASE_HOMOZYGOUS 1u
#define WHAMD_TAGPHASE_PHASED 2u
#define WHAMD_TAGPHASE_SNV 4u

typedef struct whamd_tagphase_view {
	uint64_t n_variants;
	const uint8_t* variant_flags;       /* [n_variants] WHAMD_TAGPHASE_* */
	uint64_t n_reads;
	const uint64_t* read_ptr;           /* [n_reads + 1] into the entry arrays */
	const uint32_t* entry_variant;      /* [n_entries] index of the variant */
	const uint8_t* entry_id;            /* [n_entries] 0 / 1 */
	const int32_t* entry_quality;       /* [n_entries] */
	const int64_t* read_ps;             /* [n_reads] PS_tag - 1 */
	const int32_t* read_hp;             /* [n_reads] HP_tag - 1 */
	double gap_threshold;
	uint32_t only_indels;               /* 0 / 1 */
	uint32_t want_table;                /* 0 / 1: keep every (phase set, sum0, sum1, first) row */
} whamd_tagphase_view;

typedef struct whamd_tagphase_stats {
	uint64_t n_reads;
	uint64_t n_variants;
	uint64_t n_entries;
	uint64_t n_voting;                  /* entries that vote */
	uint64_t n_skipped;                 /* reads with ps >= 0 and hp > 1 */
	uint64_t n_voted;                   /* variants with a vote */
	uint64_t n_kept;
	uint64_t n_zero_total;
	uint64_t variants_class_a;          /* voted variants of 1 .. 64 voting entries: eight lanes each */
	uint64_t variants_class_b;          /* 65 .. 4096: one wave each */
	uint64_t variants_class_c;          /* more: one workgroup each */
	uint64_t variants_many_phase_sets;  /* of them: more than 4 phase sets, one pass per phase set */
	uint64_t table_rows;                /* 0 without want_table */
	uint32_t launches;                  /* kernel launches of the whole call: 0, 7 or 11 */
	double host_ms;                     /* wall, whole call: validation, phase sets to dense ids */
	double upload_ms;                   /* HIP events, whole call */
	double kernel_ms;                   /* HIP events, whole call */
	double download_ms;                 /* HIP events, whole call */
	double total_ms;                    /* wall, whole call */
} whamd_tagphase_stats;

typedef struct whamd_tagphase_result whamd_tagphase_result; /* opaque: the result of one whamd_tagphase call */

/* One call for a batch of problems (chromosomes x samples): one upload, a constant number of launches. */
whamd_status_t whamd_tagphase(const whamd_tagphase_view* problems, uint64_t n_problems, int device, whamd_tagphase_result** out);
uint64_t whamd_tagphase_problem_count(const whamd_tagphase_result* r);
/* Variants of problem m. */
uint64_t whamd_tagphase_count(const whamd_tagphase_result* r, uint64_t m);
/* Per variant of problem m: voted (0 / 1); first, the index in the problem's entry arrays of its first voting entry (orders the
 * reference's votes and components dicts; UINT64_MAX: not voted); n_phasesets; the winner's phase set (the caller's value) and haplotype;
 * score; total; kept; zero_total.  NULL skips. */
whamd_status_t whamd_tagphase_get(const whamd_tagphase_result* r, uint64_t m, uint8_t* voted_out, uint64_t* first_out, uint32_t* n_phasesets_out,
                                  int64_t* best_ps_out, uint8_t* best_id_out, int64_t* score_out, int64_t* total_out, uint8_t* kept_out,
                                  uint8_t* zero_total_out);
/* The vote table of problem m (want_table): row_ptr_out [variants + 1]; per row the phase set, the sums of haplotype 0 and 1 and the
 * index of the phase set's first voting entry at the variant; a variant's rows ascend in `first`.  NULL skips. */
uint64_t whamd_tagphase_row_count(const whamd_tagphase_result* r, uint64_t m);
whamd_status_t whamd_tagphase_get_table(const whamd_tagphase_result* r, uint64_t m, uint64_t* row_ptr_out, int64_t* ps_out, int64_t* sum0_out,
                                        int64_t* sum1_out, uint64_t* first_out);
/* Counts of problem m; launches and times are those of the whole call. */
whamd_status_t whamd_tagphase_get_stats(const whamd_tagphase_result* r, uint64_t m, whamd_tagphase_stats* stats_out);
void whamd_tagphase_destroy(whamd_tagphase_result* r);

/* ---- Prior genotype likelihoods (compute_genotypes of src/genotyper.cpp, core.pyx:603; the loop of whatshap/cli/genotype.py:245-262) ---------
 * The first compute step of `whatshap genotype`: for every position of the list, the distribution over the genotypes 0/0, 0/1, 1/1 that
 * all reads of the sample give it; it becomes the prior of the genotyping table.  One problem is one sample on one chromosome: the
 * position list and the reads as CSR of (position, allele, quality).
 * Which entries count: for position c, in read order, every read with an entry at positions[c] whose allele is 0 or 1.  Other alleles
 * and entries at positions that are not in the list are passed over.
 * The chain: from (1/3, 1/3, 1/3); per entry p = max(0.05, pow(10.0, -(double)quality / 10.0)), allele 0 multiplies by
 * (2.0/3.0 - 1.0/3.0*p, 1.0/3.0, 1.0/3.0*p), allele 1 by the mirror image, then sum = 0.0 + d0 + d1 + d2 and d[i] /= sum; every operation
 * rounds on its own.  After the last entry the same sum once more (<= 0: three thirds).  The genotype is the first index with the
 * largest value if the other two, added in index order to 0.0, stay below 0.1; else none (-1).
 * The result depends on the order of the entries (double rounding), so the device orders every run by entry index before one lane walks
 * it: the output is bit for bit the reference's, and independent of the order in which the device's atomics arrive.
 * want_regularized: norm_sum = g0 + g1 + g2 + 3 * constant (left to right), reg[i] = (g[i] + constant) / norm_sum; reg_genotype = the
 * index of the largest reg if it is strictly greater than the second largest and than gt_prob, else -1.
 * Device (csrc/priorgt_device.hip): count per column, scan, place, order the runs (three classes by length; the last takes any length),
 * chain: WHAMD_PRIOR_GENOTYPES_LAUNCHES launches per call whatever the problems; a call without a counted entry launches nothing.
 * Errors, all with nothing launched.  WHAMD_ERR_INVALID (the message names the read): a read without entries; a read whose positions
 * are not strictly increasing; a read whose first position is smaller than that of the read before it; a read whose first or last
 * position is not in `positions`; also positions that are not strictly increasing (a duplicate, or a list that is not sorted: the
 * reference's iterator needs the order), a null array, read_ptr that decreases or does not start at 0, a constant that is negative or
 * NaN, a gt_prob that is NaN.  WHAMD_ERR_UNSUPPORTED: 2^32 - 4096 or more positions or entries in one call. */
#define WHAMD_PRIOR_GENOTYPES_LAUNCHES 8u

typedef struct whamd_prior_genotypes_view {
	uint64_t n_positions;
	const uint32_t* positions;          /* [n_positions] strictly increasing */
	uint64_t n_reads;
	const uint64_t* read_ptr;           /* [n_reads + 1] into the entry arrays */
	const uint32_t* entry_position;     /* [n_entries] */
	const uint8_t* entry_allele;        /* [n_entries] 0 / 1 count, anything else is passed over */
	const uint32_t* entry_quality;      /* [n_entries] phred, unsigned as in the reference */
	double constant;                    /* want_regularized */
	double gt_prob;                     /* want_regularized: 1 - 10^(-gt_qual_threshold / 10), computed by the caller */
	uint32_t want_regularized;          /* 0 / 1 */
	uint32_t reserved;
} whamd_prior_genotypes_view;

typedef struct whamd_prior_genotypes_stats {
	uint64_t n_reads;
	uint64_t n_positions;
	uint64_t n_entries;
	uint64_t n_counted;                 /* entries of allele 0 / 1 at a position of the list */
	uint64_t n_covered;                 /* positions with a counted entry */
	uint64_t n_genotyped;               /* positions whose genotype is not none */
	uint64_t columns_class_a;           /* covered positions of 1 .. 64 counted entries: eight lanes order each run */
	uint64_t columns_class_b;           /* 65 .. 1024: one wave, the run in LDS */
	uint64_t columns_class_c;           /* more: one workgroup, the run through LDS in tiles; any length */
	uint64_t longest_run;
	uint32_t launches;                  /* kernel launches of the whole call: 0 or WHAMD_PRIOR_GENOTYPES_LAUNCHES */
	double map_ms;                      /* wall, whole call: entry positions to columns -- done on the host, fused with the validation */
	double host_ms;                     /* wall, whole call: everything before the device (map_ms is part of it) */
	double upload_ms;                   /* HIP events, whole call */
	double kernel_ms;                   /* HIP events, whole call */
	double download_ms;                 /* HIP events, whole call */
	double total_ms;                    /* wall, whole call */
} whamd_prior_genotypes_stats;

typedef struct whamd_prior_genotypes_result whamd_prior_genotypes_result; /* opaque: the result of one whamd_prior_genotypes call */

/* One call for a batch of problems (samples x chromosomes): one upload, a constant number of launches, one download. */
whamd_status_t whamd_prior_genotypes(const whamd_prior_genotypes_view* problems, uint64_t n_problems, int device, whamd_prior_genotypes_result** out);
uint64_t whamd_prior_genotypes_problem_count(const whamd_prior_genotypes_result* r);
/* Positions of problem m. */
uint64_t whamd_prior_genotypes_count(const whamd_prior_genotypes_result* r, uint64_t m);
/* Per position of problem m: gl_out [..][3]; genotype_out 0 .. 2 or -1; with want_regularized reg_out [..][3] and reg_genotype_out
 * (without: zeros and -1).  NULL skips. */
whamd_status_t whamd_prior_genotypes_get(const whamd_prior_genotypes_result* r, uint64_t m, double* gl_out, int8_t* genotype_out, double* reg_out,
                                         int8_t* reg_genotype_out);
/* Counts of problem m; launches and times are those of the whole call. */
whamd_status_t whamd_prior_genotypes_get_stats(const whamd_prior_genotypes_result* r, uint64_t m, whamd_prior_genotypes_stats* stats_out);
void whamd_prior_genotypes_destroy(whamd_prior_genotypes_result* r);

/* ---- Polyphase threading inputs (get_allele_depths, select_clusters, compute_haplotypes of whatshap/polyphase/threading.py:274-317,
 * 228-271, 112-131) ------------------------------------------------------------------------------------------------------------------
 * What `whatshap polyphase` computes on both sides of its threader.  One problem is one block: the allele matrix (as in the read
 * scoring above: rows by local position, a position listed twice keeps the allele listed last), the clustering as CSR -- cluster c
 * lists the reads cluster_reads[cluster_ptr[c] .. cluster_ptr[c+1]-1] IN THE ORDER OF ITS LIST --, the ploidy, max_cluster_gap and the
 * number of alleles.
 * Rows: one per (position, cluster) with at least one row entry of a read of the cluster, a position's rows ascending in the cluster.
 * depth[allele] = reads of the cluster with that allele there; first[allele] = the smallest rank, in the cluster's list, of such a read
 * (UINT32_MAX: none) -- ascending `first` is the insertion order of the reference's inner dict.  consensus: `ploidy` picks, each the
 * allele with the largest (double)depth / (double)(1 + times picked), equal quotients to the smaller `first`.
 * Selection, per position: rows by total depth descending, equal depths by cluster ascending; the first always, then up to
 * min(rows, ploidy + 2) in all while (double)depth / (double)(depth of all rows) < 1.0 / (8.0 * ploidy) is false -- the first row for
 * which it is true ends the list.  Gap filling, positions 1 .. n-2 in increasing order: every cluster of the list of position - 1 (as
 * extended, in that list's order: depth order, then the order of appending) that is not in the list yet and is in the original
 * selection of one of the next min(max_cluster_gap, n - position - 1) positions is appended while the list holds fewer than ploidy + 2;
 * an appended cluster's depth row at that position, if it has one, is zeroed (its consensus and `first` stay).  Finally every list is
 * sorted ascending; cov_rank keeps an entry's place before that sort, cov_readded marks the appended ones.
 * WHAMD_POLY_THREAD_DEPTHS_ONLY: rows only -- no selection (empty lists), positions without a row allowed.
 * Device (csrc/polythread_device.hip): count per position, scan, place, the distinct clusters of every run, scan, the rows, the
 * selection: WHAMD_POLY_THREAD_LAUNCHES launches per call whatever the problems; a call without a counted entry launches nothing.  The
 * gap filling is sequential and runs on the host after the download.
 * Errors, all with nothing launched.  WHAMD_ERR_INVALID: what the matrix refuses (see above), a ploidy below 1 or above
 * WHAMD_POLY_THREAD_MAX_PLOIDY, n_alleles below 1 or above WHAMD_POLY_THREAD_MAX_ALLELES, an allele outside 0 .. n_alleles-1, a read id
 * outside the matrix, a read in two clusters or twice in one, a position without a row (the message names it; not with DEPTHS_ONLY),
 * a null array, cluster_ptr that decreases or does not start at 0.  WHAMD_ERR_UNSUPPORTED: 2^32 - 4096 or more positions or row entries
 * in one call (every count stays inside uint32), 2^28 or more reads in one cluster. */
#define WHAMD_POLY_THREAD_MAX_PLOIDY 16u
#define WHAMD_POLY_THREAD_MAX_ALLELES 16u
#define WHAMD_POLY_THREAD_LAUNCHES 13u
#define WHAMD_POLY_THREAD_DEPTHS_ONLY 1u

typedef struct whamd_poly_thread_view {
	whamd_poly_matrix_view matrix;
	uint64_t n_clusters;
	const uint64_t* cluster_ptr;        /* [n_clusters + 1] */
	const uint32_t* cluster_reads;      /* [cluster_ptr[n_clusters]] read ids, in list order */
	uint32_t ploidy;
	uint32_t max_cluster_gap;
	uint32_t n_alleles;
	uint32_t flags;                     /* WHAMD_POLY_THREAD_DEPTHS_ONLY */
} whamd_poly_thread_view;

typedef struct whamd_poly_thread_stats {
	uint64_t n_reads;
	uint64_t n_positions;
	uint64_t n_entries;                 /* row entries of the matrix */
	uint64_t n_counted;                 /* of them: of reads that are in a cluster */
	uint64_t n_rows;                    /* (position, cluster) rows */
	uint64_t n_selected;                /* entries of the lists before the gap filling */
	uint64_t n_readded;                 /* entries the gap filling appended */
	uint64_t n_emptied;                 /* of them: with a depth row, now zeroed */
	uint64_t positions_class_a;         /* positions of 1 .. 64 counted entries: eight lanes each */
	uint64_t positions_class_b;         /* 65 .. 4096: one wave each */
	uint64_t positions_class_c;         /* more: one workgroup each */
	uint32_t launches;                  /* kernel launches of the whole call: 0 or WHAMD_POLY_THREAD_LAUNCHES */
	double host_ms;                     /* wall, whole call: validation, matrix rows, reads to (cluster, rank) */
	double upload_ms;                   /* HIP events, whole call */
	double kernel_ms;                   /* HIP events, whole call */
	double download_ms;                 /* HIP events, whole call */
	double fill_ms;                     /* wall, whole call: gap filling and result assembly on the host */
	double total_ms;                    /* wall, whole call */
} whamd_poly_thread_stats;

typedef struct whamd_poly_thread_result whamd_poly_thread_result; /* opaque: the result of one whamd_poly_thread_inputs call */

/* One call for a batch of problems (blocks): one upload, a constant number of launches. */
whamd_status_t whamd_poly_thread_inputs(const whamd_poly_thread_view* problems, uint64_t n_problems, int device, whamd_poly_thread_result** out);
uint64_t whamd_poly_thread_problem_count(const whamd_poly_thread_result* r);
/* Positions, rows and list entries of problem m. */
uint64_t whamd_poly_thread_position_count(const whamd_poly_thread_result* r, uint64_t m);
uint64_t whamd_poly_thread_row_count(const whamd_poly_thread_result* r, uint64_t m);
uint64_t whamd_poly_thread_cov_count(const whamd_poly_thread_result* r, uint64_t m);
/* The rows of problem m: pc_ptr_out [positions + 1]; per row the cluster, depth_out [rows][n_alleles] (after the gap filling zeroed what
 * it zeroes), first_out [rows][n_alleles], consensus_out [rows][ploidy].  NULL skips. */
whamd_status_t whamd_poly_thread_get_rows(const whamd_poly_thread_result* r, uint64_t m, uint64_t* pc_ptr_out, uint32_t* cluster_out, uint32_t* depth_out,
                                          uint32_t* first_out, int8_t* consensus_out);
/* The lists of problem m: cov_ptr_out [positions + 1]; per entry the cluster (ascending within a position), readded (0 / 1) and rank (its
 * place in the position's list before the final sort).  NULL skips. */
whamd_status_t whamd_poly_thread_get_cov(const whamd_poly_thread_result* r, uint64_t m, uint64_t* cov_ptr_out, uint32_t* cluster_out, uint8_t* readded_out,
                                         uint32_t* rank_out);
/* Counts of problem m; launches and times are those of the whole call. */
whamd_status_t whamd_poly_thread_get_stats(const whamd_poly_thread_result* r, uint64_t m, whamd_poly_thread_stats* stats_out);
void whamd_poly_thread_destroy(whamd_poly_thread_result* r);

/* The selection and the gap filling alone, from a (position, cluster, total depth) CSR as select_clusters is handed it: position p lists
 * pc_cluster[pc_ptr[p] .. pc_ptr[p+1]-1], distinct, in any order -- equal depths go to the cluster listed earlier (the reference's stable
 * sort over dict order).  The selection is the kernel of whamd_poly_thread_inputs (one launch), the filling its host function.
 * Outputs: cov_ptr_out [n_pos + 1]; cluster / readded / rank [n_pos * (ploidy + 2)], the first cov_ptr_out[n_pos] used.
 * WHAMD_ERR_INVALID: a position without a cluster, a cluster listed twice at a position, two or more clusters of total depth 0 (the
 * reference divides by zero), a position's depths summing beyond uint32, a ploidy outside 1 .. WHAMD_POLY_THREAD_MAX_PLOIDY. */
whamd_status_t whamd_poly_select_clusters(uint64_t n_pos, const uint64_t* pc_ptr, const uint32_t* pc_cluster, const uint32_t* pc_total, uint32_t ploidy,
                                          uint32_t max_cluster_gap, int device, uint64_t* cov_ptr_out, uint32_t* cluster_out, uint8_t* readded_out,
                                          uint32_t* rank_out, uint32_t* launches_out);

/* compute_haplotypes over arrays (one launch): paths [n_pos][ploidy] cluster ids; the rows as above with consensus [rows][ploidy];
 * haplotypes_out [ploidy][n_pos]: slot i at p gets pick number (earlier slots of p with the same cluster) of that cluster's consensus, -1
 * where the cluster has no row at p. */
whamd_status_t whamd_poly_haplotypes(const uint32_t* paths, uint64_t n_pos, uint32_t ploidy, const uint64_t* pc_ptr, const uint32_t* pc_cluster,
                                     const int8_t* pc_consensus, int device, int8_t* haplotypes_out, uint32_t* launches_out);

/* ---- Polyphase threading DP (HaploThreader::computePaths of src/polyphase/haplothreader.cpp, as compute_threading_path calls it) ---------
 * What lies between whamd_poly_select_clusters and whamd_poly_haplotypes.  One problem: the lists (cov_map) as CSR, any order within a
 * position; per (position, cluster) row the total depth -- every listed cluster needs a row at its position, a re-added cluster one of
 * depth 0 --; ploidy, the two switch costs, max_cluster_gap, block_starts (sections [block_starts[i], block_starts[i+1]), the last to the
 * end; empty ones are skipped), row_limit (0 only).  The sections of all problems of a call are the jobs.
 * Per column the tuples (multisets of `ploidy` clusters of the position's list) in the reference's enumeration order; coverage cost as
 * getCoverageCost (double sum, float once), tuples above 30 + the column's smallest left out; score(t) = min over the column before of
 * score(p) + cost(k) (float; cost(0) adds nothing), + coverage cost(t); cost(k) = float(switch_cost k + affine_switch_cost (k > 0)), k =
 * ploidy - |p and t|.  Among equal sums the equivalent tuple, then the lower predecessor score, then the lower rank (place among the
 * column's surviving tuples); the end of a section is its lowest score, then the lowest rank.  `ambiguous` of a section counts the
 * decisions along the returned path that only the rank made, plus one if the end's score is not unique: where it is 0 the path is the
 * reference's, slot order included; otherwise it is an optimal path.
 * Device (csrc/polythreader_device.hip): count, scan (2), columns (one workgroup per section), backtrace:
 * WHAMD_POLY_THREADER_LAUNCHES launches per call whatever the problems; smoothed coverages and log terms are host work inside the call.
 * Errors, all with nothing launched unless said.  WHAMD_ERR_INVALID: a ploidy outside WHAMD_POLY_THREADER_MIN_PLOIDY ..
 * WHAMD_POLY_THREADER_MAX_PLOIDY, row_limit other than 0, switch costs that are negative, NaN, not multiples of 2^-20 below 2^20 or for
 * which some cost(k) is not exact in float, an empty list, a cluster listed twice at a position, a listed cluster without a depth row
 * ("has no depth row"), block_starts that is empty, does not begin with 0 or decreases, a null array, offsets that decrease or do not
 * start at 0.  WHAMD_ERR_UNSUPPORTED: more than WHAMD_POLY_THREADER_MAX_CLUSTERS clusters at a position, smoothed coverages of a
 * position summing beyond int32, 2^32 - 4096 or more positions or tuples in one call, a backtrace store the device cannot hold (after
 * the first three launches).  Never a truncated or approximate answer. */
#define WHAMD_POLY_THREADER_MIN_PLOIDY 2u
#define WHAMD_POLY_THREADER_MAX_PLOIDY 6u
#define WHAMD_POLY_THREADER_MAX_CLUSTERS 8u
#define WHAMD_POLY_THREADER_LAUNCHES 5u
#define WHAMD_POLY_THREADER_WANT_COSTS 1u

typedef struct whamd_poly_threader_view {
	uint64_t n_positions;
	const uint64_t* cov_ptr;            /* [n_positions + 1] */
	const uint32_t* cov_cluster;        /* [cov_ptr[n_positions]] cluster ids */
	const uint64_t* pc_ptr;             /* [n_positions + 1] the depth rows */
	const uint32_t* pc_cluster;
	const uint32_t* pc_total;           /* per row: depth over all alleles */
	uint64_t n_block_starts;
	const uint64_t* block_starts;
	double switch_cost;
	double affine_switch_cost;
	uint32_t ploidy;
	uint32_t max_cluster_gap;
	uint32_t row_limit;                 /* 0 */
	uint32_t flags;                     /* WHAMD_POLY_THREADER_WANT_COSTS: keep the coverage cost of every tuple */
} whamd_poly_threader_view;

typedef struct whamd_poly_threader_stats {
	uint64_t n_positions;
	uint64_t n_sections;
	uint64_t n_tuples;                  /* of all columns */
	uint64_t n_entries;                 /* of them: within 30 of their column's smallest coverage cost (backtrace records) */
	uint32_t launches;                  /* kernel launches of the whole call: 0 or WHAMD_POLY_THREADER_LAUNCHES */
	double host_ms;                     /* wall, whole call: validation, smoothed coverages, log terms */
	double upload_ms;                   /* HIP events, whole call */
	double kernel_ms;                   /* HIP events, whole call */
	double download_ms;                 /* HIP events, whole call */
	double total_ms;                    /* wall, whole call */
} whamd_poly_threader_stats;

typedef struct whamd_poly_threader_result whamd_poly_threader_result; /* opaque: the result of one whamd_poly_threader call */

/* One call for a batch of problems: one upload, a constant number of launches. */
whamd_status_t whamd_poly_threader(const whamd_poly_threader_view* problems, uint64_t n_problems, int device, whamd_poly_threader_result** out);
uint64_t whamd_poly_threader_problem_count(const whamd_poly_threader_result* r);
/* Positions, (non-empty) sections, list entries and kept tuple costs of problem m. */
uint64_t whamd_poly_threader_position_count(const whamd_poly_threader_result* r, uint64_t m);
uint64_t whamd_poly_threader_section_count(const whamd_poly_threader_result* r, uint64_t m);
uint64_t whamd_poly_threader_cov_count(const whamd_poly_threader_result* r, uint64_t m);
uint64_t whamd_poly_threader_cost_count(const whamd_poly_threader_result* r, uint64_t m);
/* Problem m: paths_out [positions][ploidy] cluster ids in slot order; path_cost_out [positions] the coverage cost of the path's tuple;
 * smoothed_out per list entry (computeCoverage); per section its first position, its score (the optimum) and `ambiguous`;
 * all_costs_out (WANT_COSTS) the coverage cost of every tuple, positions in order, tuples in enumeration order.  NULL skips. */
whamd_status_t whamd_poly_threader_get(const whamd_poly_threader_result* r, uint64_t m, uint32_t* paths_out, float* path_cost_out, uint32_t* smoothed_out,
                                       uint64_t* section_first_out, float* score_out, uint32_t* ambiguous_out, float* all_costs_out);
/* Counts of problem m; launches and times are those of the whole call. */
whamd_status_t whamd_poly_threader_get_stats(const whamd_poly_threader_result* r, uint64_t m, whamd_poly_threader_stats* stats_out);
void whamd_poly_threader_destroy(whamd_poly_threader_result* r);

/* ---- Read merging (ReadMerger.merge of whatshap/merge.py; `whatshap phase --merge-reads`, cli/phase.py:517-534) ---------------------------
 * The step in front of the read selection.  One problem is one read set: the reads, IN THE ORDER GIVEN, as CSR of (position, allele,
 * quality); the two integer thresholds, which the caller computes with the reference's own expression, 1 + int(log(threshold, (1 - e) /
 * (e / 3))); and max_error_rate.  Read i has begin_i (the position of its first entry), len_i entries and end_i = begin_i + len_i -- a
 * position plus a count, as there.
 * Pairs: j < i are compared iff end_j > max(begin_{j+1} .. begin_i).  hang = begin_i - begin_j; start = hang if hang >= 0, else
 * max(len_j + hang, 0); L = min(len_j - start, len_i); mismatch = the t < L with allele_j[start + t] != allele_i[t] -- a shift by list
 * index, as there; match = L - mismatch.  Blue edge: L >= thr_neg_diff and (double)min(match, mismatch) / (double)L <= max_error_rate
 * and match - mismatch >= thr_diff.  A blue edge is also a not-blue edge iff mismatch - match >= thr_neg_diff.
 * Components of the blue graph, the smallest id their representative.  A component of more than one read is one superread at its
 * representative: per position of any member sum[a] = the members' qualities with allele a (int64), positions ascending, allele 0 if
 * sum0 >= sum1 else 1, quality |sum1 - sum0|.  The reference cuts components apart when not-blue edges exist (n_not_blue > 0): the
 * caller does that from the edge list and calls again with `representative` given, which skips pairs and components.
 * Device (csrc/readmerge_device.hip): the pairs -- flags and mismatches, scan, the edge list in ascending (j, i) -- and the sums
 * (integer atomics per (superread, position, allele), then allele and quality): WHAMD_READMERGE_LAUNCHES launches for a call with a pair
 * and a superread, whatever the problems; 4 of them are the pairs', 5 the superreads', and a stage without work launches nothing.  Union-find
 * and the superreads' sorted positions are host work inside the call.
 * Errors, all with nothing launched.  WHAMD_ERR_INVALID: a read without entries, an allele outside {0, 1}, a null array, read_ptr that
 * decreases or does not start at 0, a given representative that is not the smallest id of its component.  WHAMD_ERR_UNSUPPORTED: a
 * position of magnitude 2^62 or more; |quality| of a problem summing beyond 2^63 - 1; 2^32 - 4096 or more reads, entries or pairs in
 * one call.  Never an approximate answer. */
#define WHAMD_READMERGE_LAUNCHES 9u

typedef struct whamd_readmerge_view {
	uint64_t n_reads;
	const uint64_t* read_ptr;           /* [n_reads + 1] into the entry arrays */
	const int64_t* entry_position;      /* [n_entries] */
	const uint8_t* entry_allele;        /* [n_entries] 0 / 1 */
	const int64_t* entry_quality;       /* [n_entries] */
	const uint32_t* representative;     /* NULL, or [n_reads]: the components are given */
	int64_t thr_diff;
	int64_t thr_neg_diff;
	double max_error_rate;
	uint32_t want_edges;                /* 0 / 1: keep the edge list */
	uint32_t reserved;
} whamd_readmerge_view;

typedef struct whamd_readmerge_stats {
	uint64_t n_reads;
	uint64_t n_entries;
	uint64_t n_pairs;                   /* pairs compared */
	uint64_t n_blue;
	uint64_t n_not_blue;
	uint64_t n_merged_components;       /* components of more than one read */
	uint64_t n_merged_entries;          /* entries of their reads */
	uint64_t n_super_entries;           /* entries of the superreads */
	uint32_t launches;                  /* kernel launches of the whole call: 0, 4, 5 or WHAMD_READMERGE_LAUNCHES */
	double host_ms;                     /* wall, whole call: validation, packing, partner ranges */
	double upload_ms;                   /* HIP events, whole call (both stages) */
	double kernel_ms;                   /* HIP events, whole call (both stages) */
	double pair_kernel_ms;              /* of it: the pairs' four launches, the wait for the edge count included */
	double download_ms;                 /* HIP events, whole call */
	double components_ms;               /* wall, whole call: union-find, the superreads' positions and slots */
	double total_ms;                    /* wall, whole call */
} whamd_readmerge_stats;

typedef struct whamd_readmerge_result whamd_readmerge_result; /* opaque: the result of one whamd_readmerge call */

/* One call for a batch of problems (read sets): a constant number of launches. */
whamd_status_t whamd_readmerge(const whamd_readmerge_view* problems, uint64_t n_problems, int device, whamd_readmerge_result** out);
uint64_t whamd_readmerge_problem_count(const whamd_readmerge_result* r);
/* Reads, superread entries and (want_edges) edges of problem m. */
uint64_t whamd_readmerge_count(const whamd_readmerge_result* r, uint64_t m);
uint64_t whamd_readmerge_super_count(const whamd_readmerge_result* r, uint64_t m);
uint64_t whamd_readmerge_edge_count(const whamd_readmerge_result* r, uint64_t m);
/* Per read of problem m: its representative and the number of reads in its component; super_ptr_out [reads + 1]: read k owns the
 * superread entries super_ptr[k] .. super_ptr[k+1]-1 (none unless it represents more than one read); per entry the position
 * (ascending within a superread), allele, quality and the two sums.  NULL skips. */
whamd_status_t whamd_readmerge_get(const whamd_readmerge_result* r, uint64_t m, uint32_t* representative_out, uint32_t* component_size_out,
                                   uint64_t* super_ptr_out, int64_t* position_out, uint8_t* allele_out, int64_t* quality_out, int64_t* sum0_out,
                                   int64_t* sum1_out);
/* The blue edges of problem m (want_edges) in ascending (j, i): byte for byte the same from call to call.  NULL skips. */
whamd_status_t whamd_readmerge_get_edges(const whamd_readmerge_result* r, uint64_t m, uint32_t* j_out, uint32_t* i_out, uint32_t* match_out,
                                         uint32_t* mismatch_out, uint8_t* not_blue_out);
/* Counts of problem m; launches and times are those of the whole call. */
whamd_status_t whamd_readmerge_get_stats(const whamd_readmerge_result* r, uint64_t m, whamd_readmerge_stats* stats_out);
void whamd_readmerge_destroy(whamd_readmerge_result* r);

#ifdef __cplusplus
}
#endif
#endif /* WHATSHAP_AMD_H */
