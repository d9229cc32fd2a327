// polyreorder.cpp -- the host side of polyphase reordering (polyreorder.h): validation, the matrix rows (polyscore.cpp), every
// breakpoint's window and read list, the tail after the device (first largest permutation, chained assignments, permuted threads and
// haplotypes, confidences), the C ABI of whatshap_amd.h's reordering section; and, in the debug library only, the one-thread host twin of
// the two kernels (whamd_debug_poly_reorder_host).
#include "polyreorder.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "../../include/whatshap_amd_debug.h"
#include "batch_call.h"
#include "debug_build.h"

using namespace whamd;

// ---------------------------------------------------------------------------------------------- validation, windows, read lists
namespace {

// Do the affected haplotypes carry at least two values at position x?
inline bool heterozygous(const int8_t* hap, uint64_t n_pos, const uint8_t* affected, uint32_t k, uint64_t x) {
	const int8_t first = hap[(uint64_t)affected[0] * n_pos + x];
	for (uint32_t j = 1; j < k; j++)
		if (hap[(uint64_t)affected[j] * n_pos + x] != first) return true;
	return false;
}

bool ascending_from_zero(const uint64_t* ptr, uint64_t n) {
	if (ptr[0] != 0) return false;
	for (uint64_t x = 0; x < n; x++)
		if (ptr[x] > ptr[x + 1]) return false;
	return true;
}

}  // namespace

whamd_status_t whamd::reorder_prepare(const whamd_poly_reorder_view& v, ReorderProblem& p, std::string& msg) {
	if (v.ploidy == 0 || v.ploidy > PR_MAX_PLOIDY) {
		msg = "ploidy " + std::to_string(v.ploidy) + " outside 1 .. " + std::to_string(PR_MAX_PLOIDY);
		return WHAMD_ERR_INVALID;
	}
	whamd_status_t st = poly_build_matrix(v.matrix, p.m, msg);
	if (st != WHAMD_OK) return st;
	if (v.n_pos != p.m.n_positions) {
		msg = "n_pos " + std::to_string(v.n_pos) + " is not the number of positions of the matrix (" + std::to_string(p.m.n_positions) + ")";
		return WHAMD_ERR_INVALID;
	}
	const uint64_t n_pos = v.n_pos, n_bp = v.n_breakpoints, n_reads = p.m.n_reads;
	if ((n_pos && (!v.haplotypes || !v.threads)) || (v.n_clusters && !v.cluster_ptr) ||
	    (n_bp && (!v.bp_position || !v.bp_affected_ptr || !v.bp_affected || !v.bp_cluster_ptr))) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (v.n_clusters >= UINT32_MAX || n_bp >= UINT32_MAX) {
		msg = "more than 2^32 - 2 clusters or breakpoints in one problem";
		return WHAMD_ERR_UNSUPPORTED;
	}
	if (v.n_clusters) {
		if (!ascending_from_zero(v.cluster_ptr, v.n_clusters)) {
			msg = "cluster_ptr must start at 0 and not decrease";
			return WHAMD_ERR_INVALID;
		}
		const uint64_t n = v.cluster_ptr[v.n_clusters];
		if (n && !v.cluster_reads) {
			msg = "null argument";
			return WHAMD_ERR_INVALID;
		}
		for (uint64_t x = 0; x < n; x++)
			if (v.cluster_reads[x] >= n_reads) {
				msg = "read id " + std::to_string(v.cluster_reads[x]) + " of the clustering is out of range (" + std::to_string(n_reads) + " reads)";
				return WHAMD_ERR_INVALID;
			}
	}
	p.ploidy = v.ploidy;
	p.n_pos = n_pos;
	p.haplotypes = v.haplotypes;
	p.threads = v.threads;
	p.bp_pos.resize(n_bp);
	p.bp_k.resize(n_bp);
	p.bp_left.resize(n_bp);
	p.bp_affected.assign(n_bp * PR_MAX_AFFECTED, 0);
	p.win_ptr.assign(n_bp + 1, 0);
	p.item_ptr.assign(n_bp + 1, 0);
	p.llh_ptr.assign(n_bp + 1, 0);
	if (n_bp && (!ascending_from_zero(v.bp_affected_ptr, n_bp) || !ascending_from_zero(v.bp_cluster_ptr, n_bp))) {
		msg = "bp_affected_ptr and bp_cluster_ptr must start at 0 and not decrease";
		return WHAMD_ERR_INVALID;
	}
	if (n_bp && v.bp_cluster_ptr[n_bp] && !v.bp_clusters) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	std::vector<uint32_t> left;
	for (uint64_t b = 0; b < n_bp; b++) {
		const std::string where = "breakpoint " + std::to_string(b) + ": ";
		const uint64_t pos = v.bp_position[b];
		if (pos < 1 || pos >= n_pos) {
			msg = where + "position " + std::to_string(pos) + " outside [1, " + std::to_string(n_pos) + ")";
			return WHAMD_ERR_INVALID;
		}
		if (b && pos <= v.bp_position[b - 1]) {
			msg = where + "position " + std::to_string(pos) + " does not ascend";
			return WHAMD_ERR_INVALID;
		}
		const uint64_t k = v.bp_affected_ptr[b + 1] - v.bp_affected_ptr[b];
		if (k < 2 || k > PR_MAX_AFFECTED) {
			msg = where + std::to_string(k) + " affected haplotypes, outside 2 .. " + std::to_string(PR_MAX_AFFECTED);
			return WHAMD_ERR_INVALID;
		}
		uint8_t* affected = p.bp_affected.data() + b * PR_MAX_AFFECTED;
		for (uint64_t j = 0; j < k; j++) {
			const uint32_t h = v.bp_affected[v.bp_affected_ptr[b] + j];
			if (h >= v.ploidy) {
				msg = where + "affected haplotype " + std::to_string(h) + " at ploidy " + std::to_string(v.ploidy);
				return WHAMD_ERR_INVALID;
			}
			if (j && h <= affected[j - 1]) {
				msg = where + "the affected haplotypes are not sorted";
				return WHAMD_ERR_INVALID;
			}
			affected[j] = (uint8_t)h;
		}
		p.bp_pos[b] = (uint32_t)pos;
		p.bp_k[b] = (uint32_t)k;
		// the window: up to PR_WINDOW heterozygous positions below pos, up to PR_WINDOW from pos on
		left.clear();
		for (uint64_t x = pos; x-- > 0 && left.size() < PR_WINDOW;)
			if (heterozygous(v.haplotypes, n_pos, affected, (uint32_t)k, x)) left.push_back((uint32_t)x);
		p.win.insert(p.win.end(), left.rbegin(), left.rend());
		p.bp_left[b] = (uint32_t)left.size();
		uint32_t right = 0;
		for (uint64_t x = pos; x < n_pos && right < PR_WINDOW; x++)
			if (heterozygous(v.haplotypes, n_pos, affected, (uint32_t)k, x)) {
				p.win.push_back((uint32_t)x);
				++right;
			}
		p.win_ptr[b + 1] = p.win.size();
		// the reads: clusters as listed, reads in cluster order; spanning the breakpoint; not dropped by extractSubMatrix(.., true)
		const uint64_t n_win = p.win_ptr[b + 1] - p.win_ptr[b];
		const uint32_t w_first = n_win ? p.win[p.win_ptr[b]] : 0, w_last = n_win ? p.win.back() : 0;
		for (uint64_t c = v.bp_cluster_ptr[b]; c < v.bp_cluster_ptr[b + 1]; c++) {
			const uint32_t cid = v.bp_clusters[c];
			if (cid >= v.n_clusters) {
				msg = where + "cluster id " + std::to_string(cid) + " is out of range (" + std::to_string(v.n_clusters) + " clusters)";
				return WHAMD_ERR_INVALID;
			}
			if (!n_win) continue;   // (start = UINT32_MAX, end = 0: every read is dropped)
			for (uint64_t x = v.cluster_ptr[cid]; x < v.cluster_ptr[cid + 1]; x++) {
				const uint32_t r = v.cluster_reads[x];
				const uint32_t first = p.m.first[r], last = p.m.last[r];
				if (!(first < pos && pos <= last)) continue;
				if (first >= w_last || last < w_first) continue;
				p.item_read.push_back(r);
			}
		}
		p.item_ptr[b + 1] = p.item_read.size();
		if (p.item_ptr[b + 1] - p.item_ptr[b] >= UINT32_MAX) {
			msg = where + "more than 2^32 - 2 reads";
			return WHAMD_ERR_UNSUPPORTED;
		}
		p.llh_ptr[b + 1] = p.llh_ptr[b] + pr_factorial((uint32_t)k);
	}
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- the tail
void whamd::reorder_tail(const ReorderProblem& p, const ReorderScores& sc, ReorderTail& out) {
	const uint64_t n_bp = p.n_breakpoints(), n_pos = p.n_pos;
	const uint32_t ploidy = p.ploidy;
	out.best.assign(n_bp, 0);
	out.assignments.assign((n_bp + 1) * ploidy, 0);
	out.confidence.assign(n_bp, 0.0);
	for (uint32_t t = 0; t < ploidy; t++) out.assignments[t] = t;
	for (uint64_t b = 0; b < n_bp; b++) {
		const double* llh = sc.llh.data() + p.llh_ptr[b];
		const uint32_t n_perm = (uint32_t)(p.llh_ptr[b + 1] - p.llh_ptr[b]), k = p.bp_k[b];
		const uint8_t* affected = p.bp_affected.data() + b * PR_MAX_AFFECTED;
		uint32_t best = 0;
		for (uint32_t x = 1; x < n_perm; x++)
			if (llh[x] > llh[best]) best = x;   // max(d, key = d.get): the first of equals
		out.best[b] = best;
		const uint32_t* prev = out.assignments.data() + b * ploidy;
		uint32_t* next = out.assignments.data() + (b + 1) * ploidy;
		for (uint32_t t = 0; t < ploidy; t++) next[t] = prev[t];
		const uint32_t perm = pr_unrank(best, k);
		for (uint32_t i = 0; i < k; i++) {
			const uint32_t from = affected[i], to = affected[(perm >> (4 * i)) & 15u];
			for (uint32_t t = 0; t < ploidy; t++)
				if (prev[t] == from) {
					next[t] = to;
					break;
				}
		}
	}
	// permute_blocks: block i is [its breakpoint, the next one)
	out.threads.resize(n_pos * ploidy);
	out.haplotypes.resize((uint64_t)ploidy * n_pos);
	for (uint64_t i = 0; i <= n_bp; i++) {
		const uint64_t s = i ? p.bp_pos[i - 1] : 0, e = i < n_bp ? p.bp_pos[i] : n_pos;
		const uint32_t* a = out.assignments.data() + i * ploidy;
		for (uint64_t x = s; x < e; x++)
			for (uint32_t t = 0; t < ploidy; t++) {
				out.threads[x * ploidy + t] = p.threads[x * ploidy + a[t]];
				out.haplotypes[(uint64_t)t * n_pos + x] = p.haplotypes[(uint64_t)a[t] * n_pos + x];
			}
	}
	// compute_breakpoint_confidence: the linkage the assignments of the two blocks amount to, against all
	for (uint64_t b = 0; b < n_bp; b++) {
		const double* llh = sc.llh.data() + p.llh_ptr[b];
		const uint32_t n_perm = (uint32_t)(p.llh_ptr[b + 1] - p.llh_ptr[b]), k = p.bp_k[b];
		const uint8_t* affected = p.bp_affected.data() + b * PR_MAX_AFFECTED;
		const uint32_t* prev = out.assignments.data() + b * ploidy;
		const uint32_t* next = out.assignments.data() + (b + 1) * ploidy;
		bool is_affected[PR_MAX_PLOIDY] = {};
		for (uint32_t j = 0; j < k; j++) is_affected[affected[j]] = true;
		uint32_t reduced[PR_MAX_AFFECTED], n_red = 0;
		for (uint32_t t = 0; t < ploidy; t++)
			if (is_affected[next[t]]) reduced[n_red++] = next[t];
		uint32_t link = 0, n_link = 0;   // as indices into `affected`
		for (uint32_t t = 0; t < ploidy; t++)
			if (is_affected[prev[t]]) {
				uint32_t at = 0;
				while (reduced[at] != prev[t]) ++at;
				link |= at << (4 * n_link++);
			}
		const double best = llh[out.best[b]];
		double sum = 0.0;
		for (uint32_t x = 0; x < n_perm; x++) sum += std::exp(llh[x] - best);
		out.confidence[b] = std::exp(llh[pr_rank(link, k)] - best) / sum;
	}
}

// ---------------------------------------------------------------------------------------------- host twin (debug library)
#ifdef WHAMD_DEBUG_BUILD
void whamd::reorder_score_host(const ReorderProblem& p, double log_match, double log_err, ReorderScores& out) {
	out.llh.assign(p.llh_ptr.back(), 0.0);
	std::vector<double> table;
	for (uint64_t b = 0; b < p.n_breakpoints(); b++) {
		const uint32_t k = p.bp_k[b];
		const uint8_t* affected = p.bp_affected.data() + b * PR_MAX_AFFECTED;
		const uint64_t n_items = p.item_ptr[b + 1] - p.item_ptr[b];
		table.assign(n_items * 2 * k, 0.0);
		for (uint64_t x = 0; x < n_items; x++) {
			const uint32_t r = p.item_read[p.item_ptr[b] + x];
			const uint64_t rb = p.m.row_ptr[r];
			pr_read_rows(p.m.row_pos.data() + rb, p.m.row_allele.data() + rb, (uint32_t)(p.m.row_ptr[r + 1] - rb), p.win.data() + p.win_ptr[b],
			             (uint32_t)(p.win_ptr[b + 1] - p.win_ptr[b]), p.bp_pos[b], p.haplotypes, p.n_pos, affected, k, log_match, log_err,
			             table.data() + x * 2 * k);
		}
		const uint32_t n_perm = pr_factorial(k);
		for (uint32_t rank = 0; rank < n_perm; rank++) {
			const uint32_t perm = pr_unrank(rank, k);
			double acc = 0.0;
			for (uint64_t x = 0; x < n_items; x++) acc += pr_read_term(table.data() + x * 2 * k, k, perm);
			out.llh[p.llh_ptr[b] + rank] = acc;
		}
	}
}
#endif

// ---------------------------------------------------------------------------------------------- C ABI
struct whamd_poly_reorder_result {
	struct Problem {
		uint32_t ploidy = 0;
		std::vector<uint64_t> llh_ptr, win_ptr;
		std::vector<uint32_t> win, left;
		std::vector<double> llh;
		ReorderTail tail;
		whamd_poly_reorder_stats stats{};
	};
	std::vector<Problem> problems;
};

namespace {

whamd_status_t reorder(const whamd_poly_reorder_view* views, uint64_t n, double log_match, double log_err, int device, bool host,
                       whamd_poly_reorder_result** out) {
	return run_batch<ReorderProblem, ReorderScores>(
		views, n, host, out, reorder_prepare,
		[&](auto& problems, auto& scores) {
			for (size_t x = 0; x < problems.size(); x++) reorder_score_host(problems[x], log_match, log_err, scores[x]);
		},
		[&](auto& problems, auto& scores, CallTimes& times, std::string& msg) { return reorder_score_device(problems, log_match, log_err, device, scores, times, msg); },
		[](ReorderProblem& p, ReorderScores& sc, whamd_poly_reorder_result::Problem& o) {
			reorder_tail(p, sc, o.tail);
			o.ploidy = p.ploidy;
			o.stats.n_breakpoints = p.n_breakpoints();
			o.stats.n_reads_visited = p.item_read.size();
			o.stats.n_permutations = p.llh_ptr.back();
			o.stats.n_window_positions = p.win.size();
			o.llh_ptr = std::move(p.llh_ptr);
			o.win_ptr = std::move(p.win_ptr);
			o.win = std::move(p.win);
			o.left = std::move(p.bp_left);
			o.llh = std::move(sc.llh);
		});
}

}  // namespace

extern "C" {

whamd_status_t whamd_poly_reorder(const whamd_poly_reorder_view* problems, uint64_t n_problems, double log_match, double log_err, int device,
                                  whamd_poly_reorder_result** out) {
	return guarded([&]() -> whamd_status_t { return reorder(problems, n_problems, log_match, log_err, device, false, out); });
}

uint64_t whamd_poly_reorder_problem_count(const whamd_poly_reorder_result* r) { return r ? r->problems.size() : 0; }

uint64_t whamd_poly_reorder_breakpoint_count(const whamd_poly_reorder_result* r, uint64_t m) {
	const auto* p = problem_of(r, m);
	return p ? p->left.size() : 0;
}

uint64_t whamd_poly_reorder_llh_count(const whamd_poly_reorder_result* r, uint64_t m) {
	const auto* p = problem_of(r, m);
	return p ? p->llh.size() : 0;
}

uint64_t whamd_poly_reorder_window_count(const whamd_poly_reorder_result* r, uint64_t m) {
	const auto* p = problem_of(r, m);
	return p ? p->win.size() : 0;
}

whamd_status_t whamd_poly_reorder_get_llh(const whamd_poly_reorder_result* r, uint64_t m, uint64_t* llh_ptr_out, double* llh_out, uint32_t* best_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	copy_out(llh_ptr_out, p->llh_ptr);
	copy_out(llh_out, p->llh);
	copy_out(best_out, p->tail.best);
	return WHAMD_OK;
}

whamd_status_t whamd_poly_reorder_get_windows(const whamd_poly_reorder_result* r, uint64_t m, uint64_t* window_ptr_out, uint32_t* left_count_out,
                                              uint32_t* position_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	copy_out(window_ptr_out, p->win_ptr);
	copy_out(left_count_out, p->left);
	copy_out(position_out, p->win);
	return WHAMD_OK;
}

whamd_status_t whamd_poly_reorder_get_phasing(const whamd_poly_reorder_result* r, uint64_t m, uint32_t* assignments_out, int32_t* threads_out,
                                              int8_t* haplotypes_out, double* confidence_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	copy_out(assignments_out, p->tail.assignments);
	copy_out(threads_out, p->tail.threads);
	copy_out(haplotypes_out, p->tail.haplotypes);
	copy_out(confidence_out, p->tail.confidence);
	return WHAMD_OK;
}

whamd_status_t whamd_poly_reorder_get_stats(const whamd_poly_reorder_result* r, uint64_t m, whamd_poly_reorder_stats* stats_out) {
	return get_stats_of(r, m, stats_out);
}

void whamd_poly_reorder_destroy(whamd_poly_reorder_result* r) { delete r; }

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_poly_reorder_host(const whamd_poly_reorder_view* problems, uint64_t n_problems, double log_match, double log_err,
                                             whamd_poly_reorder_result** out) {
	return guarded([&]() -> whamd_status_t { return reorder(problems, n_problems, log_match, log_err, 0, true, out); });
}
#endif

}  // extern "C"
