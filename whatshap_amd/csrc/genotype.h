// genotype.h -- GenotypeDPTable: the forward-backward genotyper that shares the phasing
// path's columns, indexing scheme and pedigree partitions (src/genotypedptable.cpp:16-451) -- sum-product instead of
// min-plus, no backtrace, no ties.  f64 arithmetic (the reference computes in long double, so parity is to a relative tolerance, not
// bit-exact).  Files: genotype.cpp (the model), genotype_plan.h / genotype_plan.cpp (host planning of both device paths, no HIP calls),
// genotype_slots.hip (the run-fused path), genotype_device.hip (path selection, the per-column path, the column store kept between calls).
#pragma once
#include <string>
#include <vector>

#include "device_runtime.h"
#include "problem.h"

namespace whamd {

struct GenotypeStats {
	uint64_t n_columns = 0, n_cells = 0;   // sum_c 2^k_c
	uint64_t launches = 0;
	double backward_ms = 0, forward_ms = 0, total_ms = 0;   // HIP events: checkpoint pass / windows (recompute + forward) / all
	uint32_t window = 0;                   // columns per window (backward columns kept at window ends, recomputed inside)
	uint32_t max_coverage = 0, transmissions = 0;
	uint32_t slot_runs = 0;                // run-fused path: launches per chain (0: per-column kernels)
};

// Per-column model of the genotyper, built on the host from a Problem (columns_only):
//   transition_bern  [n_cols][2 * triples + 1]  normalised Bernoulli terms: P(i -> j) = bern[popcount(i ^ j)]
//                    (TransitionProbabilityComputer, src/transitionprobabilitycomputer.cpp:22-45)
//   allele_prior     [n_cols][T][A]             P(allele assignment a | transmission value i) from the genotype priors
//                    (:48-90: product of the individuals' priors, divided by the multiplicity of the genotype vector, normalised)
//   error_prob       [entries]                  10^(-phred / 10), 0.9999 for phred 0 (src/genotypecolumncostcomputer.cpp:26-48)
struct GenotypeModel {
	uint32_t A = 0;                 // allele assignments = 2^P
	std::vector<double> transition_bern, allele_prior, error_prob;
	std::vector<uint8_t> genotype_index;   // [T][A][n_ind]: allele0 + allele1 of individual under (i, a)  (:376-383)
};
whamd_status_t build_genotype_model(const Problem& p, GenotypeModel& m, std::string& msg);

// gl_out: [n_ind][n_cols][3] genotype likelihoods (0/0, 0/1, 1/1), each triple normalised to sum 1
// (GenotypeDPTable::get_genotype_likelihoods, src/genotypedptable.cpp:444-451).  Picks the path: the run-fused one wherever it applies (no forced
// window, WHAMD_GENOTYPE_COLUMNS not set, the table eligible), else the per-column kernels.
whamd_status_t genotype_solve(const Problem& p, const GenotypeModel& m, int device, uint32_t window_hint,
                              std::vector<double>& gl_out, GenotypeStats& st, std::string& msg);

// The per-column path (genotype_device.hip): one launch per column and direction, backward columns kept per window of `window_hint` columns
// (0: chosen from the free memory).  The device is open and T is 1, 4 or 16 (genotype_solve).
whamd_status_t genotype_solve_columns(const Problem& p, const GenotypeModel& m, int device, uint32_t window_hint,
                                      std::vector<double>& gl_out, GenotypeStats& st, std::string& msg);

// The run-fused path (genotype_slots.hip): slot runs with sums instead of minima, both chains side by side, one combine launch.
// `used` = false (and WHAMD_OK): take the per-column kernels -- the table is not eligible, or the f64 range ran out inside a run (a column's
// scaled total below GS_MIN_TOTAL, genotype_plan.h) and what was written to gl_out / st is to be discarded.
whamd_status_t genotype_solve_slots(const Problem& p, const GenotypeModel& m, int device, std::vector<double>& gl_out, GenotypeStats& st,
                                    bool& used, std::string& msg);

// What a path starts from: gl_out all zero, the stats that follow from the problem alone (n_columns, transmissions, n_cells, max_coverage).
void genotype_begin(const Problem& p, std::vector<double>& gl_out, GenotypeStats& st);

// Free memory of the current device as a solve may count on it: idle arenas of the phasing path are released first when less than half is
// free, and the column store kept from an earlier call counts as free.
whamd_status_t genotype_free_bytes(int device, size_t& free_bytes, std::string& msg);

// Frees the device memory the solves keep between calls (one column store per device); device_release_caches() calls it.
void genotype_release_cache();
// The column store kept between calls (mapping tens of GB of fresh device memory took seconds in one call out of four):
// acquire returns the cached block of `device` grown to `bytes` and marks it in use, or nullptr (in use by another call,
// allocation failed, caching disabled) -- the caller then allocates its own.  release marks it idle again; a block larger than
// a quarter of the device's memory is freed instead of kept (a later phasing solve sizes its arena from what is free).
void* genotype_slab_acquire(int device, size_t bytes);
void genotype_slab_release(int device);
size_t genotype_slab_idle_bytes(int device);
// A call's hold on the acquired block (`device` >= 0): released on every way out.  Declared before the call's Session, so that the
// session has waited for its stream by then.
struct GenotypeSlabHold {
	int device = -1;
	~GenotypeSlabHold() { if (device >= 0) genotype_slab_release(device); }
};

// What the call object of either path starts from: the hold, the session, and the three ways a solve gets device memory.
struct GenotypeCall {
	GenotypeSlabHold slab;   // (before the session, see above)
	Session ses;             // the call's streams, events and blocks: given back whichever way the call ends
	hipError_t alloc(void** dptr, size_t bytes) { return ses.fresh_block(dptr, bytes); }
	hipError_t up(void** dptr, const void* src, size_t bytes);   // a fresh block and the copy into it, on the session's stream
	hipError_t take_store(void** dptr, size_t bytes);            // the column store: the block kept between calls, or a fresh one
};

}  // namespace whamd
