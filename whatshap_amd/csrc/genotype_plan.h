// genotype_plan.h -- the host side of the genotyper's two device paths (genotype.h), free of HIP calls (genotype_plan.cpp is compiled as
// host code; tests/test_genotype_plan_host.py includes this header alone):
//   run path (genotype_slots.hip):          the descriptors its kernels read, and GenoRunPlan: which runs, where their tables and columns lie,
//                                           which runs rescale, how the runs are cut into windows when the column stores exceed their budget;
//   per-column path (genotype_device.hip):  the grid of a column kernel, the window choice, the memory estimate, the founder / child slots.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "slots.h"

namespace whamd {

struct GenotypeModel;

// ---------------------------------------------------------------------------------------------- run path: what the kernels read
// Uploaded as raw bytes: the layout of the four structs is part of the kernels' ABI.
constexpr int GS_MAXLOCAL = 12;      // local slots of a run (<= 6 lane + 3 wave)

// Per column: which reads end / start in it (local slots, the order does not matter for sums) and which slots hold a read.
struct GsCol {
	uint32_t active;                 // slots (local and grid) that hold a read in this column
	uint8_t n_end, n_start, first_of_table, last_of_table;
	uint8_t end_slot[GS_MAXLOCAL], start_slot[GS_MAXLOCAL];
};
static_assert(sizeof(GsCol) == 32, "GsCol layout");
// Per column: the read in every slot (tables kernel and combine kernel only).
struct GsRow {
	double pe[SLOT_MAXSLOTS];        // error probability of the read's entry (src/genotypecolumncostcomputer.cpp:26-48)
	uint8_t ind[SLOT_MAXSLOTS + 2];
	uint8_t allele[SLOT_MAXSLOTS + 2];   // 0 REF, 1 ALT, 2 BLANK
};
static_assert(sizeof(GsRow) == 264, "GsRow layout");
// Per run.
struct GsRun {
	uint32_t c0, ncols, g, L, lw, threads, has_prev, has_next;
	uint32_t in_occ, in_identity, out_occ, pad0;
	uint32_t in_pos[8], out_pos[8];      // entry / exit index bit of every slot (SlotRun)
	unsigned long long tab_off;          // tables of the run: G [2^g][ncols][T][E], V [2^lw][ncols][T][E], S [ncols][64][E]  (doubles, E = 2 P)
	unsigned long long store_off;        // the run's columns in the two column stores: [ncols][2^g * threads] doubles
	uint32_t v_off, s_off;               // V and S relative to tab_off
	uint32_t part_in_f, part_out_f, part_in_b, part_out_b;   // first per-workgroup partial sum of the exchange columns read / written (forward, backward)
	uint32_t n_part_in_f, n_part_in_b;   // how many (0: this run does not rescale; geno_wire_rescaling)
	uint32_t emit_f, emit_b;             // 1: the neighbour rescales, leave the per-workgroup sum of what is handed on
};
static_assert(sizeof(GsRun) == 168, "GsRun layout");
// The f64 range between two rescalings.  A chain multiplies every cell by S(x) <= 1 per column and is never rescaled inside a launch (a run spans
// 2^g workgroups: no maximum across them).  Measured with the long-double restatement (oracle/genotype_oracle.py returns log10 of the column
// totals its normalisation divides out; DESIGN.md has the table): the total of a column shrinks by 1e-1.1 per column on the synthetic generator at
// coverage 6, by 1e-1.8 with phred-93 qualities, by 1e-2.1 .. 1e-8.8 per column on conflict-rich tables and by 1e-6.3 under priors of 1e-30 against
// the reads -- over ONE run of 32 columns by 1e-46, 1e-92 (1e-119 in a table of 3000 columns) and 1e-101 .. 1e-337 -- and the combine kernel
// multiplies the two chains.  Rescaling a chain every fourth run, the two chains at different runs, the factor applied to what a run hands on
// (the first schedule), let the product carry seven runs: 1e-205 for the generator, NaN from phred 93 on.  Hence:
//   every run rescales on entry, in both directions (GS_RESCALE = 1): a run starts from a total of 1, and the scaled total of a column of the
//     combine, sum f * b * cost * prior, is the shrink of that column's own run alone (the totals divided out of the two chains make up the rest of
//     the table's constant probability): 1e-44 at worst for the generator, 1e-87 at phred 93 (1e-118 in the long table), 1e-107 at 10 % errors.
//     With GS_RESCALE = R the runs form groups [k R, (k + 1) R) that both chains rescale on entering: the product carries one group, never two;
//   geno_slot_finish sees that total (tot[0]) for every column.  Below GS_MIN_TOTAL = 1e-150 -- or zero, or NaN -- it raises a flag, the host
//     discards the result and the table takes the per-column kernels, which normalise every column.  The stored chains are bounded by it: a
//     column's forward total and backward total are each >= tot[0] / (growth of the other chain inside the run, (1 - r)^(-2 triples) per column:
//     at most 1e88 over 32 columns of a quartet at recombination cost 1 -- no overflow either).
//   1e-150 splits the exponent range of f64 in two: a run may shrink the totals by 150 decades, and every cell within 1e-158 of its column's total
//     is still a normal number with all its digits (the per-column path keeps cells down to 1e-308 of the total, the reference 1e-4932).
constexpr uint32_t GS_RESCALE = 1;       // runs per group; both chains rescale when they enter a group
constexpr double GS_MIN_TOTAL = 1e-150;  // scaled column totals below this: the run path hands the table over
// The partial sums a run reads are the ones its neighbour writes (part_out_* and g are filled in): a forward run rescales when it is
// the first of a group, a backward run when it is the last of one.
inline void geno_wire_rescaling(std::vector<GsRun>& runs) {
	const size_t n_runs = runs.size();
	for (size_t ri = 0; ri < n_runs; ++ri) {
		GsRun& r = runs[ri];
		if (ri > 0 && ri % GS_RESCALE == 0) {
			r.part_in_f = runs[ri - 1].part_out_f; r.n_part_in_f = 1u << runs[ri - 1].g;
			runs[ri - 1].emit_f = 1;
		}
		if (ri + 1 < n_runs && (ri + 1) % GS_RESCALE == 0) {
			r.part_in_b = runs[ri + 1].part_out_b; r.n_part_in_b = 1u << runs[ri + 1].g;
			runs[ri + 1].emit_b = 1;
		}
	}
}
// Per column, for the combine kernel: blockIdx.y = column, blockIdx.x = 256-thread block of the column's lanes.
struct GsCombineCol {
	unsigned long long tab_off, store_off;   // the column's run
	uint32_t v_off, s_off;
	uint32_t ci, ncols, g, L, threads, n_blocks;
};
static_assert(sizeof(GsCombineCol) == 48, "GsCombineCol layout");
constexpr uint32_t GS_COMBINE_LANES = 8;    // lanes of a column one thread of the combine kernel goes through (one reduction for all of them)
constexpr uint32_t GS_COMBINE_BATCH = 512;  // columns per combine launch

// Dynamic LDS of a run kernel (geno_slot_run): exchange 2 x [threads] doubles | A [waves][ncols][T][E] | prior [ncols][T][A] | rho [ncols] |
// reduction scratch | GsCol [ncols].
inline size_t run_lds_bytes(uint32_t threads, uint32_t ncols, uint32_t T, uint32_t E, uint32_t A) {
	const size_t waves = threads >> 6;
	return ((size_t)2 * threads + waves * ncols * T * E + (size_t)ncols * T * A + ((ncols + 1) & ~1u) + 16) * 8 + (size_t)ncols * sizeof(GsCol);
}
// What a run kernel may take of the 160 KiB (CU_LDS_BYTES): the planner (slot_plan.cpp, genotype_mode) ends a run before it needs more -- a quartet's run of 32
// columns and four waves would need 197 KiB, it gets 24 columns --, geno_plan_windows refuses a plan that needs more all the same.
constexpr size_t GS_MAX_LDS = RUN_LDS_BUDGET;

// ---------------------------------------------------------------------------------------------- run path: windows
// Runs [r0, r1) = columns [c0, c1); `words` doubles in each of the two column stores.
struct GsWindow { size_t r0, r1; unsigned long long words; uint32_t c0, c1; };
struct GenoWindowCut {
	std::vector<GsWindow> windows;              // (r0, r1, words; the columns are the planner's to fill in)
	std::vector<unsigned long long> store_off;  // of every run, relative to its window's stores
	unsigned long long window_words = 0;        // the largest window
	bool run_too_large = false;                 // a single run exceeds the budget: nothing above is valid
};
// Consecutive runs are packed into windows of at most `budget_words` doubles per store; a run is never split.
inline GenoWindowCut geno_cut_windows(const std::vector<unsigned long long>& run_words, unsigned long long budget_words) {
	GenoWindowCut cut;
	cut.store_off.resize(run_words.size());
	GsWindow cur{0, 0, 0, 0, 0};
	for (size_t ri = 0; ri < run_words.size(); ++ri) {
		const unsigned long long words = run_words[ri];
		if (words > budget_words) { cut.run_too_large = true; return cut; }
		if (cur.words + words > budget_words) {
			cur.r1 = ri;
			cut.windows.push_back(cur);
			cur = GsWindow{ri, ri, 0, 0, 0};
		}
		cut.store_off[ri] = cur.words;
		cur.words += words;
	}
	cur.r1 = run_words.size();
	cut.windows.push_back(cur);
	for (const GsWindow& w : cut.windows) cut.window_words = std::max(cut.window_words, w.words);
	return cut;
}

// ---------------------------------------------------------------------------------------------- run path: the plan of one call
struct GenoRunPlan {
	std::vector<GsCol> cols;           // by column
	std::vector<GsRow> rows;           // by column
	std::vector<GsRun> runs;
	std::vector<GsCombineCol> ccols;   // by column
	std::vector<GsWindow> windows;
	unsigned long long tab_words = 0, window_words = 0;   // all runs' tables; one column store of the largest window
	uint32_t n_partials = 0;           // per-workgroup partial sums of the exchange columns, both directions
	uint32_t max_f = 0;                // widest exchange column: 2^max_f cells
	uint32_t max_blocks = 1;           // most combine blocks of a column
	size_t max_lds = 0;                // largest run_lds_bytes
	size_t n_sets = 1;                 // (forward store, backward store) pairs: 2 with more than one window
};
// Runs and descriptors of `p`, the wiring of the partial sums (geno_wire_rescaling).  false: the table is not eligible for the run path (a pedigree the
// planner does not cover, a column that fits no run, more reads starting / ending in a column than a run kernel loops over).
bool geno_plan_runs(const Problem& p, const GenotypeModel& m, int l_pref, GenoRunPlan& pl);
// The windows, for `free_bytes` of device memory and at most `cap_words` doubles per column store (~0: no cap).  false: not eligible (a run kernel
// needs more LDS than there is, a single run exceeds the store budget).
bool geno_plan_windows(GenoRunPlan& pl, uint32_t T, uint32_t A, size_t free_bytes, unsigned long long cap_words);

// ---------------------------------------------------------------------------------------------- per-column path
constexpr int GENO_BLOCK = 256;
constexpr uint32_t GENO_LOOP_BITS = 2;       // a thread loops over at most 4 cells of its projection entry
constexpr uint32_t GENO_GROUP_BITS = 7;      // reads per lookup table
constexpr uint32_t GENO_GROUP = 1u << GENO_GROUP_BITS;

inline uint32_t blocks_for(uint32_t k, uint32_t proj, uint32_t T) {   // grid of a column kernel: 2^(k - min(k - proj, LOOP)) entries x T threads
	const uint32_t nfree = k - proj, loop_bits = std::min(nfree, GENO_LOOP_BITS);
	const uint64_t threads = (1ull << (k - loop_bits)) * T;
	return (uint32_t)((threads + GENO_BLOCK - 1) / GENO_BLOCK);
}

// Window = how many backward columns are kept at once.  If all of them fit in a quarter of the free memory there is one window and no column is
// computed twice; otherwise the reference's scheme: sqrt(n) kept columns, the rest recomputed.  A hint is taken as given.
// per_column: bytes of one kept column (values, per-block sums, per-block likelihood sums).
inline uint32_t geno_column_window(uint32_t n, uint32_t hint, double per_column, double free_bytes) {
	uint32_t K = hint;
	if (!K) K = 2.0 * per_column * n <= 0.4 * free_bytes ? n : (uint32_t)std::ceil(std::sqrt((double)n));   // (backward AND forward columns kept)
	return std::max(1u, std::min(K, n));
}

// Device bytes of a per-column solve with windows of K columns (an estimate from above: the caller refuses what does not leave 1 GiB free).
inline double geno_column_need(uint32_t n, uint32_t K, size_t buf_doubles, uint32_t max_blocks, uint32_t n_gl, size_t n_entries, uint32_t T, uint32_t A,
                               uint32_t max_k, uint32_t n_ind) {
	const uint32_t n_windows = (n + K - 1) / K;
	return (double)(buf_doubles * 8 + (size_t)max_blocks * 8) * (n_windows + 2.0 * K + 4.0) + (double)K * max_blocks * n_gl * 8 + (double)n_entries * 10 + (double)n * (64 + 8.0 * T * A)
	       + (double)n * ((max_k + GENO_GROUP_BITS - 1) / GENO_GROUP_BITS) * GENO_GROUP * 4 * n_ind * 8.0;
}

// Product slots of the column kernels: founders first, in partition order (slot p = the haplotype that IS partition p), then the two haplotypes
// of every child.  slot_of[individual * 2 + haplotype]; child_part[i][q] = partition child slot q joins under transmission value i.
struct GenoSlotTable {
	uint32_t n_child_slots = 0;
	uint8_t slot_of[2 * MAX_IND] = {};
	uint8_t child_part[MAX_T][4] = {};
};
whamd_status_t geno_slot_table(const Problem& p, GenoSlotTable& out, std::string& msg);

}  // namespace whamd
