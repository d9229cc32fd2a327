// polyreorder.h -- the reordering phase of polyphase without prephasing (run_reordering, whatshap/polyphase/reorder.py:139-194, on
// compute_link_likelihoods :220-292, get_heterozygous_pos_for_haps :351-376, get_optimal_assignments :398-407, permute_blocks :497-511 and
// compute_breakpoint_confidence :514-527), restated from its behaviour.  The host (polyreorder.cpp) validates, builds the matrix rows
// (polyscore.h), finds every breakpoint's window and the reads that count there, in the order the reference walks them; the device
// (polyreorder_device.hip) fills the table of left / right log likelihoods per (read of a breakpoint, affected haplotype) and sums it per
// permutation; the host picks the permutations, chains the assignments, permutes threads and haplotypes and computes the confidences.
// The debug library does the device's part on one host thread with the same inline functions (below).
//
// Bits: everything up to the table is integer counting; a table value is log_match * (overlap - errors) + log_err * errors with the two
// products and the sum rounded one by one (pr_llh: no fused multiply-add); a permutation's value starts at +0.0 and takes the reads' terms
// in read order, one add each.  A read's term is the first largest left[i] + right[perm[i]] (Python's max keeps the earlier of equals).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"
#include "polyscore.h"

#ifndef WHAMD_HD
#if defined(__HIPCC__)
#define WHAMD_HD __host__ __device__
#else
#define WHAMD_HD
#endif
#endif

namespace whamd {

constexpr uint32_t PR_MAX_PLOIDY = 16;
constexpr uint32_t PR_MAX_AFFECTED = 8;     // 8! = 40 320 permutations; a permutation is eight nibbles of one word
constexpr uint32_t PR_WINDOW = 32;          // heterozygous positions per side (reorder.py:240)
constexpr uint32_t PR_BLOCK = 256;          // threads per workgroup of both kernels; the permutation kernel: one permutation per thread
constexpr uint32_t PR_READ_TILE = 256;      // reads whose table rows one LDS tile holds: 256 x 2 x 8 doubles = 32 KiB

// One breakpoint of the call as the kernels see it.
struct PrBreakpoint {
	uint64_t hap_base;      // the problem's haplotypes [ploidy][n_pos] in the haplotype piece
	uint64_t n_pos;
	uint64_t win_begin;     // its window positions (ascending) in the window piece
	uint64_t item_begin;    // its reads in the item piece
	uint64_t tab_begin;     // its table rows: n_items x {left[k], right[k]} doubles
	uint64_t llh_begin;     // its k! results
	uint32_t n_items, n_win, pos, k;
	uint32_t tile_begin;    // first workgroup of the permutation kernel
	uint32_t n_perm;        // k!
	uint8_t affected[PR_MAX_AFFECTED];
};
// One read that counts at one breakpoint: its de-duplicated row (sorted local positions, alleles) in the row pieces.
struct PrItem {
	uint64_t row_begin;
	uint32_t row_n;
	uint32_t bp;
};

WHAMD_HD inline uint32_t pr_factorial(uint32_t k) {
	uint32_t f = 1;
	for (uint32_t i = 2; i <= k; i++) f *= i;
	return f;
}

// The permutation of 0 .. k-1 with lexicographic rank `rank` (the order of itertools.permutations of a sorted list): element i in bits
// 4i .. 4i+3.
WHAMD_HD inline uint32_t pr_unrank(uint32_t rank, uint32_t k) {
	uint64_t unused = 0x76543210ull;   // the elements not yet placed, ascending, one per nibble
	uint32_t out = 0, f = pr_factorial(k);
	for (uint32_t i = 0; i < k; i++) {
		f /= k - i;
		const uint32_t d = rank / f;
		rank -= d * f;
		out |= (uint32_t)((unused >> (4 * d)) & 15u) << (4 * i);
		unused = (unused & ((1ull << (4 * d)) - 1)) | ((unused >> (4 * d + 4)) << (4 * d));
	}
	return out;
}

// The inverse of pr_unrank.
inline uint32_t pr_rank(uint32_t perm, uint32_t k) {
	uint32_t rank = 0, f = pr_factorial(k);
	for (uint32_t i = 0; i < k; i++) {
		f /= k - i;
		const uint32_t e = (perm >> (4 * i)) & 15u;
		uint32_t below = 0;
		for (uint32_t j = i + 1; j < k; j++) below += ((perm >> (4 * j)) & 15u) < e;
		rank += below * f;
	}
	return rank;
}

// log_match * (overlap - errors) + log_err * errors as the reference's Python evaluates it: three roundings.  hipcc contracts a * b + c
// into a fused multiply-add by default, in device code through __dmul_rn / __dadd_rn as well (the HIP headers define them as plain
// operators): contraction is switched off for this function, on both sides.  (g++ builds the host side for the sanitizer test only:
// x86-64 without -mfma has no fused instruction to contract into.)
WHAMD_HD inline double pr_llh(double log_match, double log_err, uint32_t overlap, uint32_t errors) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double a = log_match * (double)(overlap - errors);
	const double b = log_err * (double)errors;
	return a + b;
}

// One read at one breakpoint: over the read's alleles at window positions, per affected haplotype the llh left of `pos` to out[0 .. k)
// and from `pos` on to out[k .. 2k).  row_pos is sorted, win is sorted and not empty; hap: the problem's [ploidy][n_pos].
WHAMD_HD inline void pr_read_rows(const uint32_t* row_pos, const uint8_t* row_allele, uint32_t row_n, const uint32_t* win, uint32_t n_win, uint32_t pos,
                                  const int8_t* hap, uint64_t n_pos, const uint8_t* affected, uint32_t k, double log_match, double log_err, double* out) {
	uint32_t l_olp = 0, r_olp = 0;
	uint32_t l_err[PR_MAX_AFFECTED], r_err[PR_MAX_AFFECTED];
#pragma unroll
	for (uint32_t j = 0; j < PR_MAX_AFFECTED; j++) l_err[j] = r_err[j] = 0;
	const uint32_t w_first = win[0], w_last = win[n_win - 1];
	uint32_t lo = 0, hi = row_n;
	while (lo < hi) {   // the read's first entry at or after the window's first position
		const uint32_t mid = (lo + hi) >> 1;
		if (row_pos[mid] < w_first) lo = mid + 1;
		else hi = mid;
	}
	for (uint32_t x = lo; x < row_n; x++) {
		const uint32_t p = row_pos[x];
		if (p > w_last) break;
		uint32_t a = 0, b = n_win;
		while (a < b) {   // is p a window position?
			const uint32_t mid = (a + b) >> 1;
			if (win[mid] < p) a = mid + 1;
			else b = mid;
		}
		if (a == n_win || win[a] != p) continue;
		const bool left = p < pos;
		const int allele = (int)row_allele[x];
		l_olp += left;
		r_olp += !left;
#pragma unroll
		for (uint32_t j = 0; j < PR_MAX_AFFECTED; j++)
			if (j < k) {
				const uint32_t e = allele != (int)hap[(uint64_t)affected[j] * n_pos + p];
				l_err[j] += left ? e : 0u;
				r_err[j] += left ? 0u : e;
			}
	}
#pragma unroll
	for (uint32_t j = 0; j < PR_MAX_AFFECTED; j++)
		if (j < k) {
			out[j] = pr_llh(log_match, log_err, l_olp, l_err[j]);
			out[k + j] = pr_llh(log_match, log_err, r_olp, r_err[j]);
		}
}

// One read's term of a permutation: the first largest left[i] + right[perm[i]]; lr: the read's table row {left[k], right[k]}.
WHAMD_HD inline double pr_read_term(const double* lr, uint32_t k, uint32_t perm) {
	double best = -__builtin_inf();
	for (uint32_t i = 0; i < k; i++) {
		const double v = lr[i] + lr[k + ((perm >> (4 * i)) & 15u)];
		if (v > best) best = v;
	}
	return best;
}

// One validated problem: the matrix rows, and per breakpoint the window and the reads that count, in the reference's order.
struct ReorderProblem {
	PolyMatrix m;
	uint32_t ploidy = 0;
	uint64_t n_pos = 0;
	const int8_t* haplotypes = nullptr;   // the caller's
	const int32_t* threads = nullptr;     // the caller's
	std::vector<uint32_t> bp_pos, bp_k, bp_left;          // per breakpoint: position, affected haplotypes, window positions left of it
	std::vector<uint8_t> bp_affected;                     // [n_breakpoints][PR_MAX_AFFECTED]
	std::vector<uint64_t> win_ptr, item_ptr, llh_ptr;     // [n_breakpoints + 1]
	std::vector<uint32_t> win;                            // window positions
	std::vector<uint32_t> item_read;                      // read ids
	uint64_t n_breakpoints() const { return bp_pos.size(); }
};

struct ReorderScores {
	std::vector<double> llh;   // [llh_ptr.back()]
};

// What the host derives from the llh values (reorder.py:398-407, 497-527).
struct ReorderTail {
	std::vector<uint32_t> best;          // per breakpoint: rank of the first largest llh
	std::vector<uint32_t> assignments;   // [n_breakpoints + 1][ploidy]
	std::vector<int32_t> threads;        // [n_pos][ploidy]
	std::vector<int8_t> haplotypes;      // [ploidy][n_pos]
	std::vector<double> confidence;      // per breakpoint
};

whamd_status_t reorder_prepare(const whamd_poly_reorder_view& v, ReorderProblem& p, std::string& msg);
void reorder_tail(const ReorderProblem& p, const ReorderScores& sc, ReorderTail& out);
#ifdef WHAMD_DEBUG_BUILD
void reorder_score_host(const ReorderProblem& p, double log_match, double log_err, ReorderScores& out);
#endif

// All problems of a call: one upload, the table kernel (if any read counts anywhere) and the permutation kernel, one download.  No
// breakpoint in any problem: nothing touches the device (launches = 0).
whamd_status_t reorder_score_device(const std::vector<ReorderProblem>& ps, double log_match, double log_err, int device, std::vector<ReorderScores>& out,
                                    CallTimes& times, std::string& msg);

}  // namespace whamd
