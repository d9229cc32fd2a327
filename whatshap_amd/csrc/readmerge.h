// readmerge.h -- the compute of `whatshap phase --merge-reads`: ReadMerger.merge (whatshap/merge.py), restated from its behaviour.  Reads
// are taken in the order given; read i has begin_i (the position of its first variant), len_i variants and end_i = begin_i + len_i (a
// position plus a count, as there).  Read j < i is compared with i iff end_j > max(begin_{j+1}, ..., begin_i): the partners of j are the
// contiguous range j+1 .. hi_j.  The overlap follows Python's slice rule on LIST INDICES: hang = begin_i - begin_j, start = hang if
// hang >= 0 else max(len_j + hang, 0), L = min(len_j - start, len_i); mismatch counts the t < L with allele_j[start + t] != allele_i[t].
// A pair is a blue edge iff L >= thr_neg_diff, (double)min(match, mismatch) / (double)L <= max_error_rate and match - mismatch >=
// thr_diff; a blue edge is also a not-blue edge iff mismatch - match >= thr_neg_diff.  Reads are grouped by the components of the blue
// graph (smallest id = representative); a component of more than one read becomes one superread: per position the sums z[0], z[1] of
// the members' qualities by allele, positions ascending, allele = z[0] >= z[1] ? 0 : 1, quality = |z[1] - z[0]|.
//
// Host (readmerge.cpp): validation, begin / len / word offset per read, the alleles packed 64 per word, hi_j; after the pair kernels
// the union-find and the member lists of the components of more than one read.
// Device (readmerge_device.hip): the pairs (flags and mismatches, scan, edges in ascending (j, i)) and the superreads: a slot per
// (component, position) with an entry -- the entry that holds a position first in its component is flagged, the flags are scanned, an
// entry's slot is the number of flagged entries of its component at smaller positions ("touched" is never read off a sum) --, integer
// atomics into the slots, then allele and quality per slot.  The debug library does both in plain loops on one host thread, the pairs
// with the same functions (rm_overlap, rm_mismatches, rm_flags, rm_decide).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"

#if defined(__HIPCC__)
#define WHAMD_HD __host__ __device__
#else
#define WHAMD_HD
#endif

namespace whamd {

constexpr uint32_t RM_LAUNCHES_PAIRS = 4;   // flags, scan (2), edges
constexpr uint32_t RM_LAUNCHES_SUMS = 5;    // first, scan (2), place and add, decide
constexpr uint32_t RM_LAUNCHES = RM_LAUNCHES_PAIRS + RM_LAUNCHES_SUMS;   // a call with pairs and with a superread, whatever the batch; a stage without work launches nothing
static_assert(RM_LAUNCHES == WHAMD_READMERGE_LAUNCHES, "the header documents the constant");
constexpr uint64_t RM_MAX_COUNT = 0xfffff000ull;            // reads, entries, words, pairs of one call: below this (uint32 indices with room to round grids up)
constexpr int64_t RM_MAX_POSITION = (int64_t)1 << 62;       // |position| below this: begin + len and begin_i - begin_j stay inside int64
constexpr uint32_t RM_BLUE = 1, RM_NOT_BLUE = 2;            // RmEdge::flags, and the flag word per pair

struct RmRead {
	int64_t begin;
	uint32_t len;
	uint32_t word;   // first word of the read's packed alleles
};
struct RmEdge {
	uint32_t j, i, match, mismatch, flags;
};
struct RmThresholds {
	int64_t thr_diff, thr_neg_diff;
	double max_error_rate;
};

WHAMD_HD inline uint32_t rm_popcount(uint64_t x) {
	return (uint32_t)__builtin_popcountll(x);   // (v_bcnt on the device)
}

// The overlap's length for the pair (j, i), j compared with i, and where it starts in j.
WHAMD_HD inline uint32_t rm_overlap(const RmRead& rj, const RmRead& ri, uint32_t& start) {
	const int64_t hang = ri.begin - rj.begin;
	int64_t s;
	if (hang >= 0)
		s = hang < (int64_t)rj.len ? hang : (int64_t)rj.len;   // (a compared pair has hang < len_j)
	else
		s = (int64_t)rj.len + hang > 0 ? (int64_t)rj.len + hang : 0;
	start = (uint32_t)s;
	const uint32_t rest = rj.len - start;
	return rest < ri.len ? rest : ri.len;
}

// Mismatches over the overlap: the words of j funnel-shifted by start mod 64 against those of i, the tail word masked to L.
WHAMD_HD inline uint32_t rm_mismatches(const uint64_t* words, const RmRead& rj, const RmRead& ri, uint32_t start, uint32_t L) {
	const uint64_t* wj = words + rj.word + (start >> 6);
	const uint64_t* wi = words + ri.word;
	const uint32_t sh = start & 63u, nq = (L + 63u) >> 6;
	const uint32_t left = ((rj.len + 63u) >> 6) - (start >> 6);   // words of j from wj on
	uint32_t mismatch = 0;
	uint64_t cur = nq ? wj[0] : 0;
	for (uint32_t q = 0; q < nq; q++) {
		const uint64_t next = q + 1 < left ? wj[q + 1] : 0;
		const uint64_t x = sh ? (cur >> sh) | (next << (64u - sh)) : cur;
		const uint32_t bits = L - 64u * q;
		const uint64_t mask = bits >= 64u ? ~0ull : ((1ull << bits) - 1ull);
		mismatch += rm_popcount((x ^ wi[q]) & mask);
		cur = next;
	}
	return mismatch;
}

// The three tests and the not-blue test: RM_BLUE, RM_BLUE | RM_NOT_BLUE or 0.  The quotient is one IEEE double division.
WHAMD_HD inline uint32_t rm_flags(uint32_t L, uint32_t mismatch, const RmThresholds& t) {
	const int64_t match = (int64_t)L - (int64_t)mismatch, mis = (int64_t)mismatch;
	if (L == 0 || (int64_t)L < t.thr_neg_diff) return 0;
	const double quotient = (double)(match < mis ? match : mis) / (double)L;
	if (!(quotient <= t.max_error_rate)) return 0;
	if (match - mis < t.thr_diff) return 0;
	return mis - match >= t.thr_neg_diff ? (RM_BLUE | RM_NOT_BLUE) : RM_BLUE;
}

// A superread's entry from its two sums: ties, 0 / 0 included, keep allele 0 with quality 0.
WHAMD_HD inline void rm_decide(int64_t z0, int64_t z1, uint8_t& allele, int64_t& quality) {
	allele = z0 >= z1 ? 0 : 1;
	quality = z1 >= z0 ? z1 - z0 : z0 - z1;
}

// One validated problem.
struct ReadmergeProblem {
	const whamd_readmerge_view* view = nullptr;
	uint64_t n_reads = 0, n_entries = 0, n_words = 0, n_pairs = 0;
	bool given = false;                    // the view brings its representatives: no pairs, no union-find
	bool want_edges = false;
	RmThresholds thr{0, 0, 0.0};
	std::vector<RmRead> reads;             // word: local to the problem
	std::vector<uint64_t> words;           // packed alleles, every read from a fresh word
	std::vector<uint64_t> pair_ptr;        // [n_reads + 1]: read j's pairs are (j, j + 1 .. hi_j)
};

// What the two stages make for one problem.
struct ReadmergeScores {
	std::vector<RmEdge> edges;             // blue edges, ascending (j, i), ids local to the problem
	std::vector<uint32_t> representative;  // [n_reads]
	std::vector<uint32_t> comp_size;       // [n_reads] reads in the read's component
	// the components of more than one read, by ascending representative; the members of each by ascending id
	std::vector<uint32_t> merged_reps;
	std::vector<uint64_t> member_ptr;      // [merged components + 1] into members
	std::vector<uint32_t> members;         // read ids
	uint64_t n_merged_entries = 0;
	// the superreads
	std::vector<uint64_t> super_ptr;       // [n_reads + 1]: a representative of more than one read owns slots
	std::vector<int64_t> slot_position;    // ascending within a superread
	std::vector<int64_t> sums;             // [slots][2]
	std::vector<uint8_t> allele;           // [slots]
	std::vector<int64_t> quality;          // [slots]
	uint64_t n_not_blue = 0;
};

whamd_status_t readmerge_prepare(const whamd_readmerge_view& v, ReadmergeProblem& p, std::string& msg);

// After the edges: union-find (or the given representatives), component sizes, the members of the components of more than one read.
void readmerge_components(const ReadmergeProblem& p, ReadmergeScores& sc);

// The pairs of all problems of a call: one upload, RM_LAUNCHES_PAIRS launches (none when the call has no pair).
whamd_status_t readmerge_pairs_device(const std::vector<ReadmergeProblem>& ps, int device, std::vector<ReadmergeScores>& out, CallTimes& times, std::string& msg);
// The sums of all problems of a call: one upload, RM_LAUNCHES_SUMS launches (none when no read is merged).
whamd_status_t readmerge_sums_device(const std::vector<ReadmergeProblem>& ps, int device, std::vector<ReadmergeScores>& out, CallTimes& times, std::string& msg);

}  // namespace whamd
