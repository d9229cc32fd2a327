// progeny.h -- marker pair scoring of polyphasegenetic: ProgenyGenotypeLikelihoods::get{SimplexNulliplex,SimplexSimplex,DuplexNulliplex}Score
// (src/polyphase/progenygenotypelikelihoods.cpp:116-149) under the loop of get_variant_scoring (whatshap/polyphase/offspringscoring.py:143-188),
// and get_most_likely_variant_type (:191-211), restated from their behaviour.  The host (progeny.cpp) validates, computes the weight vectors
// and the stride list, walks every anchor's partners once to find which entries are stored and which row each of them really reads
// (the prev_variant / prev_score reuse), and repacks the table; one lane per stored entry then walks the samples in order in double
// (progeny_device.hip).  The debug library runs the same inner functions on one host thread.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"
#include "host_parallel.h"

#if defined(__HIPCC__)
#define WHAMD_HD __host__ __device__
#else
#define WHAMD_HD
#endif

namespace whamd {

constexpr uint32_t PROGENY_KIND_SN = 0, PROGENY_KIND_S2 = 1, PROGENY_KIND_DN = 2, PROGENY_KIND_INF = 3;

// The weight vectors of one ploidy (progenygenotypelikelihoods.cpp:27-69), by score kind: simplex-nulliplex (4 cases), simplex-simplex and
// duplex-nulliplex (6 cases).  `start` = log(1.0 / (ploidy - 1)).
struct ProgenyWeights {
	double same[3][6], diff[3][6];
	double start;
};
void progeny_weights(uint32_t ploidy, ProgenyWeights& w);

// The stride list of get_variant_scoring (offspringscoring.py:149-154) for scoring_window >= 1.
std::vector<uint32_t> progeny_strides(uint32_t window);

// One score: getLogLikelihoodDifference(pos1 = a, pos2 = b) over all samples.  `a` / `b` point at genotype 0 of sample 0 of the two rows;
// sample s, genotype g of a row is row[s * sample_stride + g * genotype_stride] (the caller's table: sample_stride = ploidy + 1,
// genotype_stride = 1; the packed device table: 3 * n_nodes and n_nodes).  Row a is indexed by the pair's first genotype (0 .. 2), row b
// by the second (0 .. 1).  Every product and sum is rounded on its own (no fused multiply-add), so that host and device, and the
// reference built for x86-64, form the same arguments of log; the zero-weight terms stay (they decide inf / NaN inputs).
WHAMD_HD inline double progeny_pair_score(const float* a, const float* b, uint64_t sample_stride, uint64_t genotype_stride, uint32_t n_samples,
                                          const double* same, const double* diff, uint32_t n_cases, double start) {
#pragma clang fp contract(off)
	double total = start;
	for (uint32_t s = 0; s < n_samples; s++) {
		const float* ra = a + s * sample_stride;
		const float* rb = b + s * sample_stride;
		const double a0 = (double)ra[0], b0 = (double)rb[0];
		if (a0 < 0.0 || b0 < 0.0) continue;   // no data for this sample at one of the positions
		const double a1 = (double)ra[genotype_stride], a2 = (double)ra[2 * genotype_stride], b1 = (double)rb[genotype_stride];
		// genotypePairs: (0,0) (0,1) (1,0) (1,1) (2,0) (2,1)
		const double g0 = a0 * b0, g1 = a0 * b1, g2 = a1 * b0, g3 = a1 * b1;
		double co = 0.0, dis = 0.0;
		co = co + g0 * same[0]; dis = dis + g0 * diff[0];
		co = co + g1 * same[1]; dis = dis + g1 * diff[1];
		co = co + g2 * same[2]; dis = dis + g2 * diff[2];
		co = co + g3 * same[3]; dis = dis + g3 * diff[3];
		if (n_cases > 4) {
			const double g4 = a2 * b0, g5 = a2 * b1;
			co = co + g4 * same[4]; dis = dis + g4 * diff[4];
			co = co + g5 * same[5]; dis = dis + g5 * diff[5];
		}
		if (co * dis > 0) total = total + log(co / dis);
	}
	return total;
}

// get_most_likely_variant_type's llh of one (row, parental type): `row` points at genotype 0 of sample 0, sample s at row + s * (k + 1);
// prior: [k + 1].  Starts at 1.0 (as the reference does).
WHAMD_HD inline double progeny_type_llh(const float* row, uint32_t n_samples, uint32_t k1, const double* prior) {
#pragma clang fp contract(off)
	double llh = 1.0;
	for (uint32_t s = 0; s < n_samples; s++) {
		const float* r = row + (uint64_t)s * k1;
		if ((double)r[0] < 0.0) continue;
		double likelihood = 0.0;
		for (uint32_t g = 0; g < k1; g++) likelihood = likelihood + prior[g] * (double)r[g];
		if (likelihood <= 0.0) llh = llh - HUGE_VAL;
		else llh = llh + log(likelihood);
	}
	return llh;
}

// memcpy on the worker pool for arrays of tens of megabytes (entry lists, results): one thread per 4 MB, at most host_threads().
inline void progeny_copy(void* dst, const void* src, size_t bytes) {
	parallel_ranges(bytes, host_threads(bytes, (uint64_t)4 << 20), [&](uint64_t b, uint64_t e, uint32_t) {
		if (e > b) std::memcpy((char*)dst + b, (const char*)src + b, e - b);
	});
}

// One validated problem and its entry list, in triangular order (by hi, then lo; hi > lo).
struct ProgenyProblem {
	const float* gl = nullptr;            // the caller's table [n_positions + ...][n_samples][ploidy + 1]
	uint64_t n_positions = 0, n_nodes = 0;
	uint32_t n_samples = 0, ploidy = 0;
	ProgenyWeights w;
	RawVec<uint32_t> lo, hi;              // the stored entry (anchor lo = i, partner hi = j)
	RawVec<uint32_t> eff;                 // the partner node whose row is read (j, or the earlier node of the same variant whose score is stored again)
	RawVec<uint8_t> kind;                 // PROGENY_KIND_*
	uint64_t n_inf = 0, n_reused = 0;
};

struct ProgenyResult {
	RawVec<double> score;                 // per entry
};

// Validation and the entry list.  WHAMD_ERR_INVALID with a message for ploidy < 2, scoring_window < 1, node variants outside the type arrays,
// a table at the 2^32 index limit, a partner type that has no score kind.
whamd_status_t progeny_prepare(const whamd_progeny_view& v, ProgenyProblem& p, std::string& msg);

// Row `node` of the caller's table, or `zero_row` ([n_samples * (ploidy + 1)] zeros) for a node at or beyond n_positions (getGl returns 0.0 there).
inline const float* progeny_row(const ProgenyProblem& p, uint64_t node, const float* zero_row) {
	return node < p.n_positions ? p.gl + node * p.n_samples * (uint64_t)(p.ploidy + 1) : zero_row;
}

// The device pair loop for a batch: one upload, one launch, one download.  Problems whose entries are all -inf (or that have none) are not
// uploaded; with nothing to compute nothing touches the device (times.launches = 0).
whamd_status_t progeny_score_device(const std::vector<ProgenyProblem>& ps, int device, std::vector<ProgenyResult>& out, CallTimes& times,
                                    std::string& msg);

// llh[n][(k+1)(k+2)/2] of rows[n][n_samples][k+1] (gathered by the caller) under prior[(k+1)(k+2)/2][k+1] (types in loop order g0, g1 <= g0).
whamd_status_t progeny_types_device(const float* rows, uint64_t n, uint32_t n_samples, uint32_t k1, const double* prior, int device, double* llh,
                                    std::string& msg);

}  // namespace whamd
