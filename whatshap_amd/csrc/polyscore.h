// polyscore.h -- read scoring of polyphase (ReadScoring::scoreReadset, src/polyphase/readscoring.cpp, on the AlleleMatrix of
// src/polyphase/allelematrix.cpp), restated from its behaviour.  The host (polyscore.cpp) builds the matrix, the per-position genotype
// likelihoods and the allele-pair tables, and folds them into one term table T[pos][a1][a2] (what computeLogScoreSinglePos returns for
// that position and allele pair); it also finds the candidate partners of every read.  The pair loop -- a merge over shared positions,
// one table lookup and one double add per shared position -- runs on the device (polyscore_device.hip) or, in the debug library, on
// the host with the same arithmetic.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"
#include "host_parallel.h"

namespace whamd {

// One matrix ready for the pair loop.
struct PolyMatrix {
	uint32_t n_reads = 0, n_positions = 0, max_allele = 0;
	std::vector<uint32_t> positions;      // [n_positions] sorted global positions (getPositions)
	// rows: sorted by local position, one entry per position (a position listed twice keeps the allele listed last)
	std::vector<uint64_t> row_ptr;        // [n_reads + 1]
	std::vector<uint32_t> row_pos;        // local positions
	std::vector<uint8_t> row_allele;
	std::vector<uint32_t> first, last;    // getFirstPos / getLastPos: the local index of the first / last LISTED entry (as AlleleMatrix(ReadSet*)
	                                      // takes them); an empty row has first = UINT32_MAX, last = 0 (the readList constructor's convention)
	std::vector<uint32_t> depths;         // [n_positions * max_allele]: every listed entry counts, duplicates included
	std::vector<uint32_t> order;          // reads by first position, ties by read id (std::stable_sort)
	std::vector<uint32_t> window_end;     // [n_reads]: anchor order[k] is paired with order[k+1 .. window_end[k]-1]
	std::vector<float> terms;             // [n_positions * max_allele * max_allele]
	double err = 0.0;                     // the error rate used (estimated when the caller passed 0)
	uint64_t n_candidates = 0;
};

// CSR input -> the matrix without terms or windows.  WHAMD_ERR_INVALID with a message for negative alleles, alleles above 15 (the
// reference's Genotype holds 16 alleles), positions outside uint32.
whamd_status_t poly_build_matrix(const whamd_poly_matrix_view& v, PolyMatrix& m, std::string& msg);

// estimateAlleleErrorRate (readscoring.cpp:86-107) on the depths of `m`, without printing.
double poly_estimate_error_rate(const PolyMatrix& m, uint32_t ploidy);

// The error rate (estimated if err == 0), the term table, the candidate windows.  ploidy must be at least 2 and at most 15.
void poly_prepare(PolyMatrix& m, uint32_t min_overlap, uint32_t ploidy, double err);

// float offset = -log(ploidy * (1 - 1 / ploidy)) (readscoring.cpp:62)
float poly_offset(uint32_t ploidy);

// What the pair loop returns for one matrix: entries in triangular order (i > j, by i then j), original read ids.
struct PolyResult {
	RawVec<uint32_t> i, j;
	RawVec<float> score;
	uint64_t n_overlapping = 0, n_nan = 0, n_pair_positions = 0;
};

// The pair loop of one pair (anchor row a, partner row b): the sum of the terms over shared positions in increasing order, in double.
// Returns the overlap; *sum the double sum.  Shared by the host loop and the device kernel.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t poly_pair_sum(const uint32_t* pa, const uint8_t* aa, uint64_t na, const uint32_t* pb, const uint8_t* ab, uint64_t nb,
                              const float* terms, uint32_t max_allele, double* sum) {
	// skip the anchor's entries before the partner's first position (they share nothing): binary search
	uint64_t k = 0;
	if (nb) {
		uint64_t lo = 0, hi = na;
		const uint32_t p0 = pb[0];
		while (lo < hi) {
			const uint64_t mid = (lo + hi) >> 1;
			if (pa[mid] < p0) lo = mid + 1;
			else hi = mid;
		}
		k = lo;
	}
	uint64_t l = 0;
	uint32_t ov = 0;
	double s = 0.0;
	while (k < na && l < nb) {
		const uint32_t x = pa[k], y = pb[l];
		if (x == y) {
			s += (double)terms[((uint64_t)x * max_allele + aa[k]) * max_allele + ab[l]];
			++ov; ++k; ++l;
		} else if (x < y) {
			++k;
		} else {
			++l;
		}
	}
	*sum = s;
	return ov;
}

// The host pair loop (debug library): every candidate pair of `m`, in anchor order, then sorted into triangular order.
void poly_score_host(const PolyMatrix& m, uint32_t min_overlap, float offset, PolyResult& out);

// The device pair loop for a batch of prepared matrices: one upload, one launch sequence, one download.  Matrices without candidate
// pairs are not uploaded; with none at all nothing touches the device (times.launches = 0).
whamd_status_t poly_score_device(const std::vector<PolyMatrix>& ms, uint32_t min_overlap, float offset, int device, std::vector<PolyResult>& out,
                                 CallTimes& times, std::string& msg);

}  // namespace whamd
