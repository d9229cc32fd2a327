// priorgt.h -- the first compute step of `whatshap genotype`: compute_genotypes (src/genotyper.cpp, core.pyx:603) and the loop that
// regularises its output (cli/genotype.py:245-262, determine_genotype at :55), restated from their behaviour.  For every position of the
// list the counted entries (allele 0 or 1) of all reads that cover it multiply, in read order, into a distribution over the three
// genotypes that is renormalised after every entry; the result is the prior of the genotyping table.
//
// The reads arrive read-major, the distributions are per position: the transposition runs on the device (priorgt_device.hip) as count,
// scan, place.  Unlike the sums of haplotagphase the chain is NOT independent of the order inside a run -- every step rounds three
// products, two sums and three quotients -- so the runs are put into entry order (which is read order: a read has at most one entry per
// position) before one lane walks each.  The host (priorgt.cpp) validates, maps entry positions to columns, packs (allele, quality) into
// one of 30 factor codes and builds the factor table with std::pow; the device only multiplies, adds and divides.  pg_chain and pg_tail
// below are what the kernel and the one-thread host twin of the debug library both call.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"
#include "host_parallel.h"
#include "run_scatter.h"

#if defined(__HIPCC__)
#define WHAMD_HD __host__ __device__
#else
#define WHAMD_HD
#endif

namespace whamd {

constexpr uint32_t PG_CLASS_A_MAX = 64;           // class a: 0 .. 64 counted entries, ordered by eight lanes straight from memory
constexpr uint32_t PG_CLASS_B_MAX = 1024;         // class b: 65 .. 1024, one wave with the whole run in LDS
constexpr uint32_t PG_TILE = 4096;                // class c: beyond, one workgroup; the run passes through LDS in tiles of this many (a multiple of 4) -- any length
constexpr uint32_t PG_OWN = 8;                    // class c: entries a thread ranks per pass over the run
constexpr uint32_t PG_LAUNCHES = WHAMD_PRIOR_GENOTYPES_LAUNCHES;   // count, scan (2), place, order a / b / c, chain
constexpr uint32_t PG_QUALITIES = 15;             // p = max(0.05, 10^(-q / 10)) is 0.05 from q = 14 on: 15 distinct values
constexpr uint32_t PG_CODES = 2 * PG_QUALITIES;   // code = allele * 15 + min(q, 14)
constexpr uint32_t PG_NONE = RS_NONE;             // column of an entry that is not counted

// What one column's lane writes.
struct PgOut {
	double gl[3];
	double reg[3];
	int32_t genotype;       // 0 .. 2, -1: none
	int32_t reg_genotype;
};

// The 30 factor triples, [code][3], as the reference forms them (std::pow on the host; priorgt.cpp).
void pg_factor_table(double* table);

// A column's chain: from (1/3, 1/3, 1/3), per entry d[i] *= f[i], sum = 0.0 + d0 + d1 + d2, d[i] /= sum -- GenotypeDistribution's
// operator* -- over the run's codes in order.  Every operation rounds on its own: no fused multiply-add.
WHAMD_HD inline void pg_chain(const uint8_t* codes, uint32_t n, const double* table, double (&d)[3]) {
#pragma clang fp contract(off)
	d[0] = 1.0 / 3.0;
	d[1] = 1.0 / 3.0;
	d[2] = 1.0 / 3.0;
	for (uint32_t k = 0; k < n; k++) {
		const double* f = table + 3u * codes[k];
		const double d0 = d[0] * f[0], d1 = d[1] * f[1], d2 = d[2] * f[2];
		double sum = 0.0;
		sum = sum + d0;
		sum = sum + d1;
		sum = sum + d2;
		d[0] = d0 / sum;
		d[1] = d1 / sum;
		d[2] = d2 / sum;
	}
}

// After the last entry: normalize(), likeliestGenotype() / errorProbability() < 0.1, and -- where wanted -- the regularisation and
// determine_genotype of cli/genotype.py:245-262.
WHAMD_HD inline PgOut pg_tail(const double (&d)[3], double constant, double gt_prob, bool want_reg) {
#pragma clang fp contract(off)
	PgOut o;
	double sum = 0.0;
	sum = sum + d[0];
	sum = sum + d[1];
	sum = sum + d[2];
	if (sum <= 0.0) {
		o.gl[0] = o.gl[1] = o.gl[2] = 1.0 / 3.0;
	} else {
		o.gl[0] = d[0] / sum;
		o.gl[1] = d[1] / sum;
		o.gl[2] = d[2] / sum;
	}
	int best_index = 0;
	double best = 0.0;
	for (int i = 0; i < 3; i++)
		if (o.gl[i] > best) {
			best = o.gl[i];
			best_index = i;
		}
	double err = 0.0;
	for (int i = 0; i < 3; i++)
		if (i != best_index) err = err + o.gl[i];
	o.genotype = err < 0.1 ? best_index : -1;
	o.reg[0] = o.reg[1] = o.reg[2] = 0.0;
	o.reg_genotype = -1;
	if (want_reg) {
		double norm_sum = o.gl[0] + o.gl[1];
		norm_sum = norm_sum + o.gl[2];
		norm_sum = norm_sum + 3 * constant;
		for (int i = 0; i < 3; i++) o.reg[i] = (o.gl[i] + constant) / norm_sum;
		// the largest, if it is alone at the top and above the threshold (a stable ascending sort's last two elements)
		int top = 0;
		for (int i = 1; i < 3; i++)
			if (o.reg[i] >= o.reg[top]) top = i;
		double second = -1.0;
		bool have_second = false;
		for (int i = 0; i < 3; i++)
			if (i != top && (!have_second || o.reg[i] > second)) {
				second = o.reg[i];
				have_second = true;
			}
		if (o.reg[top] > second && o.reg[top] > gt_prob) o.reg_genotype = top;
	}
	return o;
}

// One validated problem: its counted entries mapped to columns.
struct PriorProblem {
	const whamd_prior_genotypes_view* view = nullptr;
	uint64_t n_reads = 0, n_entries = 0, n_positions = 0;
	uint64_t n_counted = 0;                   // entries of allele 0 / 1 at a position of the list
	RawVec<uint32_t> column;                  // per entry: index into positions, PG_NONE: not counted
	RawVec<uint8_t> code;                     // per entry: factor code (unspecified where not counted)
	bool want_reg = false;
};

struct PriorScores {
	std::vector<PgOut> out;                   // per position
	std::vector<uint32_t> count;              // per position: counted entries
};

whamd_status_t priorgt_prepare(const whamd_prior_genotypes_view& v, PriorProblem& p, std::string& msg);

// All problems of a call: one upload, PG_LAUNCHES launches, one download, whatever the problems.  No counted entry in the whole call:
// nothing touches the device (launches = 0) and `out` stays empty -- the caller fills in the empty column's record.
whamd_status_t priorgt_device(const std::vector<PriorProblem>& ps, int device, std::vector<PriorScores>& out, CallTimes& times, std::string& msg);

}  // namespace whamd
