// progeny.h -- marker pair scoring of polyphasegenetic: ProgenyGenotypeLikelihoods::get{SimplexNulliplex,SimplexSimplex,DuplexNulliplex}Score
// (src/polyphase/progenygenotypelikelihoods.cpp:116-149) under the loop of get_variant_scoring (whatshap/polyphase/offspringscoring.py:143-188),
// and get_most_likely_variant_type (:191-211), restated from their behaviour.  The host (progeny.cpp) validates, computes the weight vectors
// and the stride list, walks every anchor's partners once to find which entries are stored and which row each of them really reads
// (the prev_variant / prev_score reuse), and repacks the table; one lane per stored entry then walks the samples in order in double
// (progeny_device.hip).  The debug library runs the same inner functions on one host thread.
// The table itself -- get_offspring_gl / compute_gt_likelihoods (:86-140, :232-274) -- is made from allele depths by progeny_gl_cell below, one device
// lane per (sample, node) cell; depths to scores is then one upload, two launches and one download (progeny_score_depths_device).
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

// ---------------------------------------------------------------------------------------------- genotype likelihoods from allele depths
// compute_gt_likelihoods (offspringscoring.py:232-274) for one cell = (depth row, sample): gl[g] = w_g / sum_g w_g with
// w_g = p_g^alt_dp * (1 - p_g)^ref_dp * prior[g]; the binomial coefficient of the reference's pmf is the same for every g and cancels.
// The powers are taken by squaring on (mantissa, binary exponent) pairs -- frexp / ldexp are exact, every product is rounded once -- so a
// weight can neither underflow nor overflow at any depth a uint32 holds; the exponents are then rebased on the largest weight, a weight
// PROGENY_GL_CUTOFF binades or more below it becomes 0, and the sum runs over g = 0 .. k in that order.  The same code runs in the debug
// library's host twin and in progeny_gl_kernel: they agree bit for bit.
// Error against the exact rational value of the doubles p_g, 1.0 - p_g and prior[g] (u = 2^-53, n = ref_dp + alt_dp): a weight carries
// (alt_dp - 1) + (ref_dp - 1) + 2 <= n roundings whichever way the squaring groups its factors, the sum k more, the division one:
//   |gl - exact| <= gamma(2n + k + 1) * exact + 2^(1 - PROGENY_GL_CUTOFF),  gamma(m) = m u / (1 - m u)        (DESIGN.md section 13).
// Divergence from the reference: where all its pmf values underflow (ZeroDivisionError, NaN) this returns the normalised values.
struct ProgenyScaled {
	double m;     // 0, or in [0.5, 1)
	int64_t e;    // the value is m * 2^e
};
constexpr int64_t PROGENY_GL_CUTOFF = 1000;

WHAMD_HD inline ProgenyScaled progeny_scaled(double x) {
	int e;
	const double m = frexp(x, &e);
	return ProgenyScaled{m, (int64_t)e};
}

WHAMD_HD inline ProgenyScaled progeny_scaled_mul(ProgenyScaled a, ProgenyScaled b) {
#pragma clang fp contract(off)
	int e;
	const double m = frexp(a.m * b.m, &e);   // the product lies in [0.25, 1): never subnormal
	return ProgenyScaled{m, a.e + b.e + e};
}

WHAMD_HD inline ProgenyScaled progeny_scaled_pow(double x, uint32_t n) {
	ProgenyScaled r{0.5, 1}, b = progeny_scaled(x);   // r = 1.0: the first product is exact
	while (n) {
		if (n & 1) r = progeny_scaled_mul(r, b);
		n >>= 1;
		if (n) b = progeny_scaled_mul(b, b);
	}
	return r;
}

// p_g: the reference's expression (get_binom_pmf), same operations in the same order.
WHAMD_HD inline double progeny_alt_probability(uint32_t g, uint32_t ploidy, double error_rate) {
#pragma clang fp contract(off)
	const double f = (double)g / (double)ploidy;
	return (1.0 - f) * error_rate + f * (1.0 - error_rate);
}

WHAMD_HD inline ProgenyScaled progeny_gl_weight(uint32_t ref_dp, uint32_t alt_dp, uint32_t g, uint32_t ploidy, double error_rate, const double* prior) {
#pragma clang fp contract(off)
	const double p = progeny_alt_probability(g, ploidy, error_rate);
	ProgenyScaled w = progeny_scaled_mul(progeny_scaled_pow(p, alt_dp), progeny_scaled_pow(1.0 - p, ref_dp));
	if (prior) w = progeny_scaled_mul(w, progeny_scaled(prior[g]));
	return w;
}

// One cell.  prior: NULL or [ploidy + 1].  Each output is optional (NULL skips): `plane` takes genotypes 0 .. 2 as float at
// plane[g * plane_stride] (the packed table progeny_pair_kernel reads), `row` all ploidy + 1 as float, `row_f64` the doubles they were
// rounded from.  A cell with fewer reads than the ploidy has no data: every value is -1, the fill value of the reference's constructor.
WHAMD_HD inline void progeny_gl_cell(uint32_t ref_dp, uint32_t alt_dp, uint32_t ploidy, double error_rate, const double* prior, float* plane,
                                     uint64_t plane_stride, float* row, double* row_f64) {
#pragma clang fp contract(off)
	if ((uint64_t)ref_dp + alt_dp < ploidy) {
		for (uint32_t g = 0; g <= ploidy; g++) {
			if (plane && g < 3) plane[g * plane_stride] = -1.0f;
			if (row) row[g] = -1.0f;
			if (row_f64) row_f64[g] = -1.0;
		}
		return;
	}
	// The weights are formed three times (largest exponent, sum, values) rather than kept: no array sized by the ploidy lives in a lane.
	bool any = false;
	int64_t top = 0;
	for (uint32_t g = 0; g <= ploidy; g++) {
		const ProgenyScaled w = progeny_gl_weight(ref_dp, alt_dp, g, ploidy, error_rate, prior);
		if (w.m > 0.0 && (!any || w.e > top)) {
			top = w.e;
			any = true;
		}
	}
	double sum = 0.0;
	for (uint32_t g = 0; g <= ploidy; g++) {
		const ProgenyScaled w = progeny_gl_weight(ref_dp, alt_dp, g, ploidy, error_rate, prior);
		sum = sum + (w.m > 0.0 && top - w.e < PROGENY_GL_CUTOFF ? ldexp(w.m, (int)(w.e - top)) : 0.0);
	}
	for (uint32_t g = 0; g <= ploidy; g++) {
		const ProgenyScaled w = progeny_gl_weight(ref_dp, alt_dp, g, ploidy, error_rate, prior);
		const double v = (w.m > 0.0 && top - w.e < PROGENY_GL_CUTOFF ? ldexp(w.m, (int)(w.e - top)) : 0.0) / sum;
		if (plane && g < 3) plane[g * plane_stride] = (float)v;
		if (row) row[g] = (float)v;
		if (row_f64) row_f64[g] = v;
	}
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
// needs_table = false: the table is made on the device (progeny_score_depths_device), v.gl is not looked at.
whamd_status_t progeny_prepare(const whamd_progeny_view& v, ProgenyProblem& p, std::string& msg, bool needs_table = true);

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

// One validated depth problem (whamd_progeny_depths_view): the arrays stay the caller's.
struct ProgenyDepths {
	const uint32_t* ref = nullptr;        // [n_samples][n_rows]
	const uint32_t* alt = nullptr;
	uint64_t n_rows = 0, n_nodes = 0;
	uint32_t n_samples = 0, ploidy = 0;
	double error_rate = 0;
	const uint32_t* node_row = nullptr;   // [n_nodes]
	const double* priors = nullptr;       // NULL or [ploidy + 1]^3
	RawVec<uint32_t> row_prior;           // with priors: [n_rows] the first double of a row's prior, (alt_count * (ploidy + 1) + co_alt_count) * (ploidy + 1)
};

// Validation.  WHAMD_ERR_INVALID with a message for ploidy < 2, an error rate outside (0, 1), a row type above the ploidy or whose prior
// row is not a distribution (priors given), a node_row entry outside the rows, a table at the 2^32 index limit.
whamd_status_t progeny_depths_prepare(const whamd_progeny_depths_view& v, ProgenyDepths& d, std::string& msg);

// The tables [n_nodes][n_samples][ploidy + 1] of a batch: one upload (depths, node_row, priors), one launch of progeny_gl_kernel, one
// download into the caller's arrays (table_out / table_f64_out: NULL, or per problem NULL or the array).
whamd_status_t progeny_gl_device(const std::vector<ProgenyDepths>& ds, int device, float* const* table_out, double* const* table_f64_out,
                                 std::string& msg);

// Depths to scores: one upload (depths and entry lists), progeny_gl_kernel writes the planes, progeny_pair_kernel reads them, one download.
// ps[x] was prepared without a table from the same view as ds[x].  As progeny_score_device, nothing touches the device when no entry
// needs a score.
whamd_status_t progeny_score_depths_device(const std::vector<ProgenyDepths>& ds, const std::vector<ProgenyProblem>& ps, int device,
                                           std::vector<ProgenyResult>& out, CallTimes& times, std::string& msg);

}  // namespace whamd
