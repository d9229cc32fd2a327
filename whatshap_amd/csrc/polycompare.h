// polycompare.h -- comparing two polyploid phasings (`whatshap compare` above ploidy 2: compare_block, compute_switch_errors_poly and
// compute_switch_flips_poly of whatshap/cli/compare.py on SwitchFlipCalculator::compare, src/polyphase/switchflipcalculator.cpp), restated
// from its behaviour.  A job is two phasings [n_pos][ploidy] and two costs; the program is a Viterbi pass over the k! permutations of the
// haplotypes per visited position: a state's cost is flip_cost times the alleles that disagree under the permutation (pc_flips), a
// transition's is switch_cost times the places in which two permutations differ (pc_switches).  The host (polycompare.cpp) validates
// and counts the matching positions; the device (polycompare_device.hip) runs one workgroup per job; the debug library runs the same
// inline functions (below) on one host thread, state by state.
//
// States and ranks: state r is the permutation of lexicographic rank r (pr_unrank: the order of std::next_permutation from the identity
// and of itertools.permutations(range(k))), element i in bits 4i .. 4i+3 -- the reference's Permutation code.
//
// Bits: a score is min over q (score[q] + switch_cost * (double)d) first, + flip_cost * (double)f after, column 0 is flip_cost * (double)f
// alone -- the reference's operation order, every product and sum rounded on its own (no fused multiply-add).  For costs whose sums are
// exact in double every score equals the reference's kept entries bit for bit; the reference's pruning never changes the optimum.
//
// The tie rule (defined HERE; the reference takes the first of equals in the iteration order of a std::unordered_map, an accident of
// libstdc++'s bucket layout, which is not reproduced): among the paths of minimum total cost the one with the fewest flips; among
// those, the predecessor of lowest rank at every step and the end state of lowest rank.  A state keeps (score, flips so far, switches
// so far); a candidate replaces the kept one when it is strictly smaller in (value, flips[q]), and the states are walked in increasing
// rank.  `switches` and `flips` depend on the input alone.
//
// One visited position: the reference's backtrace start calls getNumSwitches(row, Permutation::INVALID) without a guard for position 0;
// INVALID = 0xf000000000000000 differs from a permutation in every nibble whose value is not zero: switches = ploidy - 1.  Reproduced
// (pc_end_switches).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"
#include "polyreorder.h"

namespace whamd {

constexpr uint32_t PC_MAX_PLOIDY = 6;         // 720 states; 7! states are 25 M candidates per column, and the reference itself warns above 6
constexpr uint32_t PC_MAX_STATES = 720;
constexpr uint32_t PC_BLOCK = 256;            // threads per workgroup; a lane owns the rows lane, lane + 256, lane + 512
constexpr uint32_t PC_ROWS = 3;               // rows per lane at ploidy 6 (1 up to ploidy 5)
constexpr uint64_t PC_MAX_POSITIONS = (uint64_t)1 << 28;   // per job: ploidy * positions fits the uint32 counters
constexpr uint64_t PC_INVALID = 0xf000000000000000ull;     // Permutation::INVALID

// One job of the call as the kernel sees it.  Jobs without a visited position are not sent.
struct PcJob {
	uint64_t p0_begin, p1_begin;   // the job's phasings [n_pos][k] in the allele piece
	uint64_t n_pos, n_visited;
	uint64_t pred_begin;           // want_path: [n_visited][n_states] uint16 predecessor ranks (row 0 unused) in the predecessor block
	uint64_t path_begin;           // want_path: [n_visited] uint16 state ranks in the path block
	double switch_cost, flip_cost;
	uint32_t k, n_states, matched_only, want_path;
};
struct PcOut {
	double total;
	uint64_t min_hamming_sum;
	uint32_t switches, flips;
};

// The places in which two permutation codes differ: the reference's xor and nibble popcount (getNumSwitches).
WHAMD_HD inline uint32_t pc_switches(uint64_t a, uint64_t b) {
	const uint64_t x = a ^ b, m = 0x0111111111111111ull;
	return (uint32_t)__builtin_popcountll((x & m) | ((x >> 3) & m) | ((x >> 2) & m) | ((x >> 1) & m));
}
// The same for codes of at most eight elements.
WHAMD_HD inline uint32_t pc_switches(uint32_t a, uint32_t b) {
	const uint32_t x = a ^ b, m = 0x11111111u;
	return (uint32_t)__builtin_popcount((x & m) | ((x >> 3) & m) | ((x >> 2) & m) | ((x >> 1) & m));
}

// A position's k alleles, one per byte.
WHAMD_HD inline uint64_t pc_column(const uint8_t* p, uint32_t k) {
	uint64_t c = 0;
#pragma unroll
	for (uint32_t i = 0; i < PC_MAX_PLOIDY; i++)
		if (i < k) c |= (uint64_t)p[i] << (8 * i);
	return c;
}

// getNumFlips: how many i have phasing0[perm[i]] != phasing1[i].
WHAMD_HD inline uint32_t pc_flips(uint32_t perm, uint64_t col0, uint64_t col1, uint32_t k) {
	uint32_t f = 0;
#pragma unroll
	for (uint32_t i = 0; i < PC_MAX_PLOIDY; i++)
		if (i < k) f += ((col0 >> (8 * ((perm >> (4 * i)) & 15u))) & 255u) != ((col1 >> (8 * i)) & 255u);
	return f;
}
// getFlippedHaps as a mask: bit i set when phasing0[perm[i]] != phasing1[i].
inline uint32_t pc_flipped_mask(uint32_t perm, uint64_t col0, uint64_t col1, uint32_t k) {
	uint32_t mask = 0;
	for (uint32_t i = 0; i < k; i++) mask |= (uint32_t)(((col0 >> (8 * ((perm >> (4 * i)) & 15u))) & 255u) != ((col1 >> (8 * i)) & 255u)) << i;
	return mask;
}

// Do the two columns hold the same multiset of alleles (Genotype == Genotype)?  Every allele is as frequent in one as in the other.
WHAMD_HD inline bool pc_matched(uint64_t col0, uint64_t col1, uint32_t k) {
	bool same = true;
#pragma unroll
	for (uint32_t i = 0; i < PC_MAX_PLOIDY; i++)
		if (i < k) {
			const uint32_t a = (uint32_t)(col0 >> (8 * i)) & 255u;
			uint32_t n0 = 0, n1 = 0;
#pragma unroll
			for (uint32_t j = 0; j < PC_MAX_PLOIDY; j++)
				if (j < k) {
					n0 += ((uint32_t)(col0 >> (8 * j)) & 255u) == a;
					n1 += ((uint32_t)(col1 >> (8 * j)) & 255u) == a;
				}
			same = same && n0 == n1;
		}
	return same;
}

// The best predecessor of one row so far.
struct PcBest {
	double value;
	uint32_t flips, q;
};
WHAMD_HD inline PcBest pc_best_none() { return PcBest{__builtin_inf(), 0xFFFFFFFFu, 0u}; }

// score[q] + switch_cost * d, kept when strictly smaller in (value, flips[q]): called for q in increasing rank, the lowest rank wins.
// hipcc contracts a * b + c into a fused multiply-add by default: switched off here and in pc_state_score, on both sides.
WHAMD_HD inline void pc_consider(PcBest& best, double score_q, uint32_t flips_q, uint32_t q, double switch_cost, uint32_t d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double step = switch_cost * (double)d;
	const double v = score_q + step;
	if (v < best.value || (v == best.value && flips_q < best.flips)) best = PcBest{v, flips_q, q};
}
// Column 0: flip_cost * f alone; later columns: the minimum first, the flip term after.
WHAMD_HD inline double pc_state_score(bool first, double minimum, double flip_cost, uint32_t f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double term = flip_cost * (double)f;
	return first ? term : minimum + term;
}

// Is (score, flips) of a state of higher rank strictly better than the kept end state's?
WHAMD_HD inline bool pc_end_better(double score, uint32_t flips, double best_score, uint32_t best_flips) {
	return score < best_score || (score == best_score && flips < best_flips);
}
// The switches a job reports: the end state's sum; with one visited position what the reference's unguarded backtrace start counts.
WHAMD_HD inline uint32_t pc_end_switches(uint64_t n_visited, uint32_t end_perm, uint32_t switches_so_far) {
	return n_visited == 1 ? pc_switches((uint64_t)end_perm, PC_INVALID) : switches_so_far;
}

// One validated job.
struct CompareJob {
	uint32_t k = 0, n_states = 0;
	uint64_t n_pos = 0;
	const uint8_t* p0 = nullptr;   // the caller's
	const uint8_t* p1 = nullptr;
	double switch_cost = 0, flip_cost = 0;
	bool matched_only = false, want_path = false;
	uint64_t n_matched = 0, n_visited = 0;
};
struct CompareResult {
	PcOut out{0.0, 0, 0, 0};
	std::vector<uint16_t> path;   // want_path: the state's rank per visited position
};

whamd_status_t compare_prepare(const whamd_poly_compare_view& v, CompareJob& job, std::string& msg);
#ifdef WHAMD_DEBUG_BUILD
void compare_host(const CompareJob& job, CompareResult& out);
#endif
// All jobs of a call: one upload, one launch (one workgroup per job with a visited position; the walk back runs in the same launch), one
// download.  No visited position in any job: nothing touches the device (launches = 0).
whamd_status_t compare_device(const std::vector<CompareJob>& jobs, int device, std::vector<CompareResult>& out, CallTimes& times, std::string& msg);

}  // namespace whamd
