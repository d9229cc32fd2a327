// polythreader.h -- the threading DP of `whatshap polyphase` (HaploThreader::computePaths of src/polyphase/haplothreader.cpp), restated
// from its behaviour: per position a column over the multisets ("tuples") of `ploidy` clusters of that position's list,
//     score(t) = min over the tuples p of the column before of  (score(p) + cost(k(p, t)))  +  coverage cost(t)            (all float)
// with k = ploidy - |p and t as multisets of global ids|, cost(k) = float(switch_cost * k + affine_switch_cost * (k > 0)), cost(0) added
// as nothing at all (the reference takes the equivalent tuple's score as it is), tuples of coverage cost > 30 + the column's smallest
// left out.  DESIGN section 22 says what of the reference's result this defines and what it does not (its ties).
//
// The host makes what needs its arithmetic: the smoothed coverages (integers) and, per position, the double log terms the coverage cost
// is summed from (ph_cost).  The device (polythreader_device.hip) and the host twin (polythreader.cpp, debug library) only add; they
// share the functions below.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"
#include "run_scatter.h"

#if defined(__HIPCC__)
#define WHAMD_HD __host__ __device__
#else
#define WHAMD_HD
#endif

namespace whamd {

constexpr uint32_t PH_MIN_PLOIDY = WHAMD_POLY_THREADER_MIN_PLOIDY;
constexpr uint32_t PH_MAX_PLOIDY = WHAMD_POLY_THREADER_MAX_PLOIDY;
constexpr uint32_t PH_MAX_CLUSTERS = WHAMD_POLY_THREADER_MAX_CLUSTERS;   // per position: three bits per local id
constexpr uint32_t PH_MAX_TUPLES = 1716;                                  // C(8 + 6 - 1, 6)
constexpr uint32_t PH_MAX_TABLE = PH_MAX_CLUSTERS * PH_MAX_PLOIDY + (1u << PH_MAX_CLUSTERS);   // doubles per position
constexpr uint32_t PH_LAUNCHES = WHAMD_POLY_THREADER_LAUNCHES;           // count, scan (2), columns, backtrace
constexpr uint32_t PH_ABSENT = 8;                                         // old-to-new map: the cluster is not in the new list
constexpr uint32_t PH_PERM_BITS = 18, PH_RANK_BITS = 11, PH_TIE_BIT = 29; // a backtrace record

// Tuples of `ploidy` out of n clusters, in the order computeRelevantTuples enumerates them: non-increasing local ids v[0] >= v[1] >= ...,
// v[0] running fastest.  Each as ploidy x 3 bits, v[i] at bit 3 i.
inline void ph_enumerate(uint32_t ploidy, uint32_t n, std::vector<uint32_t>& out) {
	std::vector<uint32_t> v(ploidy, 0);
	while (v[ploidy - 1] < n) {
		uint32_t packed = 0;
		for (uint32_t i = 0; i < ploidy; i++) packed |= v[i] << (3 * i);
		out.push_back(packed);
		v[0]++;
		for (uint32_t i = 1; i < ploidy; i++)
			if (v[i - 1] >= n) v[i]++;
		for (uint32_t i = ploidy - 1; i > 0; i--)
			if (v[i - 1] >= n) v[i - 1] = v[i];
	}
}

// Where the tuples of (ploidy, n clusters) lie in the table of all of them, and how many they are.
struct PhTupleIndex {
	uint32_t begin[PH_MAX_PLOIDY + 1][PH_MAX_CLUSTERS + 1];
	uint32_t count[PH_MAX_PLOIDY + 1][PH_MAX_CLUSTERS + 1];
};
const std::vector<uint32_t>& ph_tuple_table(PhTupleIndex& index);   // polythreader.cpp: made once

// How often every local id occurs in a tuple: eight counters of four bits.
WHAMD_HD inline uint32_t ph_counts(uint32_t packed, uint32_t ploidy) {
	uint32_t c = 0;
	for (uint32_t i = 0; i < ploidy; i++) c += 1u << (4 * ((packed >> (3 * i)) & 7u));
	return c;
}

// Size of the intersection of two multisets given as counters.
WHAMD_HD inline uint32_t ph_common(uint32_t a, uint32_t b) {
	uint32_t n = 0;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		const uint32_t x = (a >> (4 * i)) & 15u, y = (b >> (4 * i)) & 15u;
		n += x < y ? x : y;
	}
	return n;
}

// getCoverageCost: the terms of the tuple's clusters in ascending local id, then the term of the reads no haplotype is threaded through,
// summed in double from 0.0, negated, rounded to float once.  tab: [n * ploidy] the term of local id c with multiplicity m at
// c * ploidy + m - 1, then [2^n] the unthreaded term by the set of threaded local ids.
WHAMD_HD inline float ph_cost(const double* tab, uint32_t ploidy, uint32_t n, uint32_t counts) {
	double llh = 0.0;
	uint32_t threaded = 0;
	for (uint32_t c = 0; c < n; c++) {
		const uint32_t m = (counts >> (4 * c)) & 15u;
		if (!m) continue;
		llh += tab[c * ploidy + m - 1];
		threaded |= 1u << c;
	}
	llh += tab[n * ploidy + threaded];
	return (float)(-llh);
}

// A tuple of the column before, in its slot order and its local ids, as counters over the new column's local ids (clusters that are
// gone match nothing).
WHAMD_HD inline uint32_t ph_counts_in_new(uint32_t old_perm, uint32_t ploidy, const uint32_t* old_to_new) {
	uint32_t c = 0;
	for (uint32_t i = 0; i < ploidy; i++) {
		const uint32_t d = old_to_new[(old_perm >> (3 * i)) & 7u];
		if (d != PH_ABSENT) c += 1u << (4 * d);
	}
	return c;
}

// TupleConverter::permuteAgainstOld: slot i keeps the cluster slot i of the predecessor had where the new tuple still holds one of it;
// the new tuple's other clusters fill the remaining slots in their order.
WHAMD_HD inline uint32_t ph_permute(uint32_t new_tuple, uint32_t old_perm, uint32_t ploidy, const uint32_t* old_to_new) {
	uint32_t v[PH_MAX_PLOIDY], u[PH_MAX_PLOIDY], rest[PH_MAX_PLOIDY], n_rest = 0;
	for (uint32_t i = 0; i < ploidy; i++) {
		v[i] = (new_tuple >> (3 * i)) & 7u;
		u[i] = 0;
	}
	for (uint32_t i = 0; i < ploidy; i++) {
		const uint32_t d = old_to_new[(old_perm >> (3 * i)) & 7u];
		bool placed = false;
		if (d != PH_ABSENT)
			for (uint32_t j = 0; j < ploidy; j++)
				if (v[j] == d) {
					u[i] = d;
					v[j] = PH_ABSENT;
					placed = true;
					break;
				}
		if (!placed) rest[n_rest++] = i;
	}
	uint32_t at = 0;
	for (uint32_t i = 0; i < ploidy; i++)
		if (v[i] != PH_ABSENT) u[rest[at++]] = v[i];
	uint32_t packed = 0;
	for (uint32_t i = 0; i < ploidy; i++) packed |= u[i] << (3 * i);
	return packed;
}

// The best predecessor so far of one tuple.  The order (the tie rule): the lowest s; among equal s the equivalent tuple
// (k = 0), then the lowest predecessor score, then the lowest rank.  Candidates come in ascending rank, so an equal one never replaces;
// it is remembered that the rank decided.
struct PhBest {
	float s, pred_score;
	uint32_t rank, equivalent, by_rank;
};
WHAMD_HD inline void ph_offer(PhBest& b, bool first, float pred_score, uint32_t k, float cost_k, uint32_t rank) {
	const float s = k ? pred_score + cost_k : pred_score;
	const uint32_t eq = k ? 0u : 1u;
	if (!first) {
		if (s > b.s) return;
		if (s == b.s) {
			if (eq < b.equivalent) return;
			if (eq == b.equivalent) {
				if (pred_score > b.pred_score) return;
				if (pred_score == b.pred_score) {
					b.by_rank = 1;
					return;
				}
			}
		}
	}
	b = PhBest{s, pred_score, rank, eq, 0};
}

// One section (a job of the call): positions [first, first + n) of the call, its ploidy, cost(k), and where its path goes.
struct PhSection {
	uint32_t first, n, ploidy, reserved;
	uint64_t path_at;              // first word of its positions in the call's paths
	float cost[PH_MAX_PLOIDY + 2];
};
struct PhSectionEnd {
	uint32_t rank, score_bits, ambiguous, reserved;
};

// One validated problem: the lists, the smoothed coverages and the log terms.
struct ThreaderProblem {
	uint32_t ploidy = 0;
	uint64_t n_pos = 0;
	bool want_costs = false;
	std::vector<uint64_t> cov_ptr;         // [n_pos + 1]
	std::vector<uint32_t> cov_cluster;     // global ids
	std::vector<uint32_t> cov_smoothed;    // clusterCoverage
	std::vector<uint64_t> tab_ptr;         // [n_pos + 1] into tab
	std::vector<double> tab;
	std::vector<std::pair<uint64_t, uint64_t>> sections;   // (first, n), the empty ones left out
	float cost[PH_MAX_PLOIDY + 2] = {};
	uint64_t n_tuples = 0;                 // of all positions
};

// Per problem, what the device (or the host twin) leaves.
struct ThreaderPaths {
	std::vector<uint32_t> paths;           // [n_pos][ploidy] global ids
	std::vector<float> path_cost;          // [n_pos] the coverage cost of the path's tuple
	std::vector<float> score;              // per section
	std::vector<uint32_t> ambiguous;
	std::vector<float> all_costs;          // want_costs: of every tuple of every position, in enumeration order
	uint64_t n_entries = 0;                // surviving tuples: the backtrace records
};

whamd_status_t polythreader_prepare(const whamd_poly_threader_view& v, ThreaderProblem& p, std::string& msg);

// All sections of all problems of a call: one upload, PH_LAUNCHES launches.
whamd_status_t polythreader_device(const std::vector<ThreaderProblem>& ps, int device, std::vector<ThreaderPaths>& out, CallTimes& times, std::string& msg);

}  // namespace whamd
