// polythreader.cpp -- the host side of the polyphase threading DP (polythreader.h): validation, computeCoverage (integers), the log terms
// of the coverage costs with the reference's arithmetic (binomial_coefficient_log, log_binom_pmf of src/binomial.cpp, restated), the
// cost(k) table, result assembly, the C ABI of whatshap_amd.h's threader section; and, in the debug library only, the one-thread host
// twin: the plain walk over all pairs of tuples of neighbouring columns.
#include "polythreader.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <unordered_map>

#include "../../include/whatshap_amd_debug.h"
#include "batch_call.h"
#include "debug_build.h"

#pragma clang fp contract(off)

using namespace whamd;

const std::vector<uint32_t>& whamd::ph_tuple_table(PhTupleIndex& index) {
	static std::vector<uint32_t> table;
	static PhTupleIndex made;
	static std::once_flag once;
	std::call_once(once, [] {
		std::memset(&made, 0, sizeof made);
		for (uint32_t ploidy = PH_MIN_PLOIDY; ploidy <= PH_MAX_PLOIDY; ploidy++)
			for (uint32_t n = 1; n <= PH_MAX_CLUSTERS; n++) {
				made.begin[ploidy][n] = (uint32_t)table.size();
				ph_enumerate(ploidy, n, table);
				made.count[ploidy][n] = (uint32_t)table.size() - made.begin[ploidy][n];
			}
	});
	index = made;
	return table;
}

namespace {

// ---------------------------------------------------------------------------------------------- the reference's log terms
double binomial_coefficient_log(int n, int k) {
	if (k < 0 || n < 0 || n < k) return 0;
	double result = 0.0;
	if (k > n - k) k = n - k;
	double buffer = 1.0;
	for (int i = 0; i < k; i++) {
		const double addition = (double)(n - i) / (double)(i + 1);
		if (buffer * addition > std::numeric_limits<double>::max()) {
			result += std::log(buffer);
			buffer = addition;
		} else {
			buffer *= addition;
		}
	}
	return result + std::log(buffer);
}

// Each distinct (n, k) once per problem; log(p) and log(1 - p) once per multiplicity.  The coefficients of one n are a row by k (a
// position asks for up to 2^8 + 48 terms of its one n), beyond 2^16 reads a map.
struct LogTerms {
	std::unordered_map<uint32_t, std::vector<double>> rows;
	std::unordered_map<uint64_t, double> sparse;
	double log_p[PH_MAX_PLOIDY + 1], log_q[PH_MAX_PLOIDY + 1];   // [0]: p = 0.025, [m]: p = (0.975 * m) / ploidy
	explicit LogTerms(uint32_t ploidy) {
		log_p[0] = std::log(0.025);
		log_q[0] = std::log(1 - 0.025);
		for (uint32_t m = 1; m <= ploidy; m++) {
			const double p = (0.975 * m) / ploidy;
			log_p[m] = std::log(p);
			log_q[m] = std::log(1 - p);
		}
	}
	std::vector<double>* row_of(uint32_t n) {
		if (n > 65536u) return nullptr;
		std::vector<double>& row = rows[n];
		if (row.empty()) row.assign((size_t)n + 1, std::numeric_limits<double>::quiet_NaN());
		return &row;
	}
	double pmf(std::vector<double>* row, uint32_t n, uint32_t k, uint32_t m) {   // log_binom_pmf(n, k, p of m)
		double coefficient;
		if (row) {
			if (std::isnan((*row)[k])) (*row)[k] = binomial_coefficient_log((int)n, (int)k);
			coefficient = (*row)[k];
		} else {
			const uint64_t key = (uint64_t)n << 32 | k;
			auto at = sparse.find(key);
			if (at == sparse.end()) at = sparse.emplace(key, binomial_coefficient_log((int)n, (int)k)).first;
			coefficient = at->second;
		}
		return coefficient + (int)k * log_p[m] + ((int)n - (int)k) * log_q[m];
	}
};

bool exact_in_float(double x) { return (double)(float)x == x; }

}  // namespace

// ---------------------------------------------------------------------------------------------- validation, coverages, terms
whamd_status_t whamd::polythreader_prepare(const whamd_poly_threader_view& v, ThreaderProblem& p, std::string& msg) {
	if (v.ploidy < PH_MIN_PLOIDY || v.ploidy > PH_MAX_PLOIDY) {
		msg = "ploidy " + std::to_string(v.ploidy) + " outside " + std::to_string(PH_MIN_PLOIDY) + " .. " + std::to_string(PH_MAX_PLOIDY);
		return WHAMD_ERR_INVALID;
	}
	if (v.row_limit != 0) {
		msg = "row_limit " + std::to_string(v.row_limit) + ": only 0 (no limit) is supported, what the pipeline passes up to ploidy 6";
		return WHAMD_ERR_INVALID;
	}
	if (v.flags & ~WHAMD_POLY_THREADER_WANT_COSTS) {
		msg = "unknown flag bits";
		return WHAMD_ERR_INVALID;
	}
	const double sc = v.switch_cost, ac = v.affine_switch_cost;
	if (!(sc >= 0) || !(ac >= 0) || std::isinf(sc) || std::isinf(ac)) {
		msg = "switch costs must be finite and not negative";
		return WHAMD_ERR_INVALID;
	}
	const uint32_t P = v.ploidy;
	p.cost[0] = 0.0f;
	for (uint32_t k = 1; k <= P; k++) {
		const double c = sc * k + ac * 1;
		if (!exact_in_float(c)) {
			msg = "cost(" + std::to_string(k) + ") = switch_cost * " + std::to_string(k) + " + affine_switch_cost is not exact in float";
			return WHAMD_ERR_INVALID;
		}
		p.cost[k] = (float)c;
	}
	const double unit = 1048576.0;   // 2^20: see DESIGN 22, the early exit
	if (sc >= unit || ac >= unit || std::floor(sc * unit) != sc * unit || std::floor(ac * unit) != ac * unit) {
		msg = "switch costs must be multiples of 2^-20 below 2^20 (the sums the reference forms in double are then exact)";
		return WHAMD_ERR_INVALID;
	}
	const uint64_t n_pos = v.n_positions;
	p.ploidy = P;
	p.n_pos = n_pos;
	p.want_costs = (v.flags & WHAMD_POLY_THREADER_WANT_COSTS) != 0;
	if (n_pos >= 0x7fffffffull) {
		msg = "2^31 - 1 or more positions";
		return WHAMD_ERR_UNSUPPORTED;
	}
	if (n_pos && (!v.cov_ptr || !v.pc_ptr)) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (!check_offsets(v.cov_ptr, n_pos, "cov_ptr", "position", msg) || !check_offsets(v.pc_ptr, n_pos, "pc_ptr", "position", msg)) return WHAMD_ERR_INVALID;
	if (n_pos && ((v.cov_ptr[n_pos] && !v.cov_cluster) || (v.pc_ptr[n_pos] && (!v.pc_cluster || !v.pc_total)))) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	// sections
	if (v.n_block_starts && !v.block_starts) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	for (uint64_t i = 0; i < v.n_block_starts; i++) {
		const uint64_t start = v.block_starts[i], end = i + 1 == v.n_block_starts ? n_pos : v.block_starts[i + 1];
		if ((i == 0 && start != 0) || start > n_pos || end < start) {
			msg = "block_starts must begin with 0, not decrease and stay within the positions";
			return WHAMD_ERR_INVALID;
		}
		if (end > start) p.sections.emplace_back(start, end - start);
	}
	if (n_pos && !v.n_block_starts) {
		msg = "block_starts is empty";
		return WHAMD_ERR_INVALID;
	}
	// the lists and every listed cluster's depth
	p.cov_ptr.assign(v.cov_ptr, v.cov_ptr + n_pos + 1);
	if (!n_pos) p.cov_ptr.assign(1, 0);
	p.cov_cluster.assign(v.cov_cluster, v.cov_cluster + p.cov_ptr[n_pos]);
	std::vector<uint32_t> depth(p.cov_cluster.size(), 0);
	PhTupleIndex index;
	ph_tuple_table(index);
	for (uint64_t x = 0; x < n_pos; x++) {
		const uint64_t b = p.cov_ptr[x], e = p.cov_ptr[x + 1];
		if (b == e) {
			msg = "position " + std::to_string(x) + ": its cov_map row is empty (the reference has no tuples there)";
			return WHAMD_ERR_INVALID;
		}
		if (e - b > PH_MAX_CLUSTERS) {
			msg = "position " + std::to_string(x) + " lists " + std::to_string(e - b) + " clusters: more than " + std::to_string(PH_MAX_CLUSTERS);
			return WHAMD_ERR_UNSUPPORTED;
		}
		for (uint64_t k = b; k < e; k++) {
			for (uint64_t j = b; j < k; j++)
				if (p.cov_cluster[j] == p.cov_cluster[k]) {
					msg = "position " + std::to_string(x) + " lists cluster " + std::to_string(p.cov_cluster[k]) + " twice";
					return WHAMD_ERR_INVALID;
				}
			const uint32_t* rb = v.pc_cluster + v.pc_ptr[x];
			const uint32_t* re = v.pc_cluster + v.pc_ptr[x + 1];
			const uint32_t* at = std::find(rb, re, p.cov_cluster[k]);
			if (at == re) {
				msg = "position " + std::to_string(x) + ": cluster " + std::to_string(p.cov_cluster[k]) + " of cov_map has no depth row";
				return WHAMD_ERR_INVALID;
			}
			depth[k] = v.pc_total[at - v.pc_cluster];
		}
		p.n_tuples += index.count[P][e - b];
	}
	// computeCoverage: per cluster the positions that list it, ascending, with running sums (uint32, wrapping as there)
	std::vector<uint32_t> ids(p.cov_cluster);
	std::sort(ids.begin(), ids.end());
	ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
	struct Seen {
		std::vector<uint32_t> pos, sum, nonzero;   // sum / nonzero: before the entry
	};
	std::vector<Seen> seen(ids.size());
	std::vector<uint32_t> dense(p.cov_cluster.size());
	for (uint64_t x = 0; x < n_pos; x++)
		for (uint64_t k = p.cov_ptr[x]; k < p.cov_ptr[x + 1]; k++) {
			dense[k] = (uint32_t)(std::lower_bound(ids.begin(), ids.end(), p.cov_cluster[k]) - ids.begin());
			Seen& s = seen[dense[k]];
			if (s.pos.empty()) {
				s.sum.push_back(0);
				s.nonzero.push_back(0);
			}
			s.pos.push_back((uint32_t)x);
			s.sum.push_back(s.sum.back() + depth[k]);
			s.nonzero.push_back(s.nonzero.back() + (depth[k] > 0 ? 1u : 0u));
		}
	p.cov_smoothed.resize(p.cov_cluster.size());
	std::vector<uint32_t> coverage(n_pos, 0);
	const uint32_t gap = v.max_cluster_gap, num_pos = (uint32_t)n_pos;
	for (uint64_t x = 0; x < n_pos; x++) {
		uint32_t lo = (uint32_t)x - gap / 2;   // (unsigned, wrapping, as there)
		const uint32_t hi = std::min(num_pos - 1, (uint32_t)x + (uint32_t)(gap + 1) / 2);
		lo *= lo < hi ? 1u : 0u;
		uint64_t total = 0;
		for (uint64_t k = p.cov_ptr[x]; k < p.cov_ptr[x + 1]; k++) {
			const Seen& s = seen[dense[k]];
			const size_t a = std::lower_bound(s.pos.begin(), s.pos.end(), lo) - s.pos.begin();
			const size_t b = std::upper_bound(s.pos.begin(), s.pos.end(), hi) - s.pos.begin();
			uint32_t sum = 0, nonzero = 0;
			if (b > a) {
				sum = s.sum[b] - s.sum[a];
				nonzero = s.nonzero[b] - s.nonzero[a];
			}
			if (!nonzero) nonzero = 1;
			p.cov_smoothed[k] = sum / nonzero;
			total += p.cov_smoothed[k];
		}
		if (total > 0x7fffffffull) {
			msg = "position " + std::to_string(x) + ": the smoothed coverages sum beyond int32";
			return WHAMD_ERR_UNSUPPORTED;
		}
		coverage[x] = (uint32_t)total;
	}
	// the terms
	LogTerms terms(P);
	p.tab_ptr.assign(n_pos + 1, 0);
	for (uint64_t x = 0; x < n_pos; x++) {
		const uint64_t n = p.cov_ptr[x + 1] - p.cov_ptr[x];
		p.tab_ptr[x + 1] = p.tab_ptr[x] + n * P + ((uint64_t)1 << n);
	}
	p.tab.resize(p.tab_ptr[n_pos]);
	for (uint64_t x = 0; x < n_pos; x++) {
		const uint32_t n = (uint32_t)(p.cov_ptr[x + 1] - p.cov_ptr[x]);
		const uint32_t* cc = p.cov_smoothed.data() + p.cov_ptr[x];
		double* tab = p.tab.data() + p.tab_ptr[x];
		std::vector<double>* row = terms.row_of(coverage[x]);
		for (uint32_t c = 0; c < n; c++)
			for (uint32_t m = 1; m <= P; m++) tab[c * P + m - 1] = terms.pmf(row, coverage[x], cc[c], m);
		double* un = tab + n * P;
		for (uint32_t threaded = 0; threaded < (1u << n); threaded++) {
			uint32_t reads = 0;
			for (uint32_t c = 0; c < n; c++)
				if (!(threaded >> c & 1u)) reads += cc[c];
			un[threaded] = terms.pmf(row, coverage[x], reads, 0);
		}
	}
	return WHAMD_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------- host twin (debug library)
#ifdef WHAMD_DEBUG_BUILD
struct TwinEntry {
	float score;
	uint32_t perm, pred, by_rank;
};

void polythreader_host(const ThreaderProblem& p, ThreaderPaths& out) {
	PhTupleIndex index;
	const std::vector<uint32_t>& table = ph_tuple_table(index);
	const uint32_t P = p.ploidy;
	out.paths.assign(p.n_pos * P, 0);
	out.path_cost.assign(p.n_pos, 0.0f);
	if (p.want_costs) {
		out.all_costs.reserve(p.n_tuples);
		for (uint64_t x = 0; x < p.n_pos; x++) {
			const uint32_t n = (uint32_t)(p.cov_ptr[x + 1] - p.cov_ptr[x]);
			const uint32_t* tt = table.data() + index.begin[P][n];
			for (uint32_t t = 0; t < index.count[P][n]; t++) out.all_costs.push_back(ph_cost(p.tab.data() + p.tab_ptr[x], P, n, ph_counts(tt[t], P)));
		}
	}
	for (const auto& sec : p.sections) {
		std::vector<std::vector<TwinEntry>> columns(sec.second);
		std::vector<float> cost;
		for (uint64_t col = 0; col < sec.second; col++) {
			const uint64_t x = sec.first + col;
			const uint32_t n = (uint32_t)(p.cov_ptr[x + 1] - p.cov_ptr[x]), nt = index.count[P][n];
			const uint32_t* tt = table.data() + index.begin[P][n];
			const double* tab = p.tab.data() + p.tab_ptr[x];
			cost.resize(nt);
			float smallest = std::numeric_limits<float>::infinity();
			for (uint32_t t = 0; t < nt; t++) {
				cost[t] = ph_cost(tab, P, n, ph_counts(tt[t], P));
				if (cost[t] < smallest) smallest = cost[t];
			}
			const float limit = 30.0f + smallest;
			uint32_t old_to_new[PH_MAX_CLUSTERS];
			if (col) {
				const uint32_t n_old = (uint32_t)(p.cov_ptr[x] - p.cov_ptr[x - 1]);
				for (uint32_t c = 0; c < n_old; c++) {
					old_to_new[c] = PH_ABSENT;
					for (uint32_t d = 0; d < n; d++)
						if (p.cov_cluster[p.cov_ptr[x] + d] == p.cov_cluster[p.cov_ptr[x - 1] + c]) old_to_new[c] = d;
				}
			}
			std::vector<TwinEntry>& column = columns[col];
			for (uint32_t t = 0; t < nt; t++) {
				if (cost[t] > limit) continue;
				if (!col) {
					column.push_back(TwinEntry{0.0f + cost[t], tt[t], 0, 0});
					continue;
				}
				const std::vector<TwinEntry>& before = columns[col - 1];
				const uint32_t mine = ph_counts(tt[t], P);
				PhBest best{};
				for (uint32_t r = 0; r < before.size(); r++) {
					const uint32_t k = P - ph_common(ph_counts_in_new(before[r].perm, P, old_to_new), mine);
					ph_offer(best, r == 0, before[r].score, k, p.cost[k], r);
				}
				column.push_back(TwinEntry{best.s + cost[t], ph_permute(tt[t], before[best.rank].perm, P, old_to_new), best.rank, best.by_rank});
			}
			out.n_entries += column.size();
		}
		// the end: the lowest score, then the lowest rank
		const std::vector<TwinEntry>& last = columns.back();
		uint32_t r = 0, ambiguous = 0, equal = 0;
		for (uint32_t k = 1; k < last.size(); k++)
			if (last[k].score < last[r].score) r = k;
		for (uint32_t k = 0; k < last.size(); k++) equal += last[k].score == last[r].score ? 1u : 0u;
		ambiguous += equal > 1 ? 1u : 0u;
		out.score.push_back(last[r].score);
		for (uint64_t col = sec.second; col-- > 0;) {
			const uint64_t x = sec.first + col;
			const uint32_t n = (uint32_t)(p.cov_ptr[x + 1] - p.cov_ptr[x]);
			const TwinEntry& e = columns[col][r];
			for (uint32_t i = 0; i < P; i++) out.paths[x * P + i] = p.cov_cluster[p.cov_ptr[x] + ((e.perm >> (3 * i)) & 7u)];
			out.path_cost[x] = ph_cost(p.tab.data() + p.tab_ptr[x], P, n, ph_counts(e.perm, P));
			ambiguous += e.by_rank;
			r = e.pred;
		}
		out.ambiguous.push_back(ambiguous);
	}
}
#endif

}  // namespace

// ---------------------------------------------------------------------------------------------- C ABI
struct whamd_poly_threader_result {
	struct Problem {
		uint32_t ploidy = 0;
		std::vector<uint32_t> paths, smoothed, ambiguous;
		std::vector<uint64_t> section_first;
		std::vector<float> path_cost, score, all_costs;
		whamd_poly_threader_stats stats{};
	};
	std::vector<Problem> problems;
};

namespace {

whamd_status_t thread_paths(const whamd_poly_threader_view* views, uint64_t n, int device, bool host, whamd_poly_threader_result** out) {
	return run_batch<ThreaderProblem, ThreaderPaths>(
		views, n, host, out, polythreader_prepare,
		[](auto& problems, auto& paths) {
			for (size_t x = 0; x < problems.size(); x++) polythreader_host(problems[x], paths[x]);
		},
		[&](auto& problems, auto& paths, CallTimes& times, std::string& msg) { return polythreader_device(problems, device, paths, times, msg); },
		[](ThreaderProblem& p, ThreaderPaths& paths, whamd_poly_threader_result::Problem& o) {
			o.ploidy = p.ploidy;
			o.paths = std::move(paths.paths);
			o.path_cost = std::move(paths.path_cost);
			o.score = std::move(paths.score);
			o.ambiguous = std::move(paths.ambiguous);
			o.all_costs = std::move(paths.all_costs);
			o.smoothed = std::move(p.cov_smoothed);
			for (const auto& s : p.sections) o.section_first.push_back(s.first);
			o.paths.resize(p.n_pos * p.ploidy);   // (a host call of the product build computes nothing)
			o.path_cost.resize(p.n_pos);
			o.score.resize(p.sections.size());
			o.ambiguous.resize(p.sections.size());
			o.stats.n_positions = p.n_pos;
			o.stats.n_sections = p.sections.size();
			o.stats.n_tuples = p.n_tuples;
			o.stats.n_entries = paths.n_entries;
		});
}

}  // namespace

extern "C" {

whamd_status_t whamd_poly_threader(const whamd_poly_threader_view* problems, uint64_t n_problems, int device, whamd_poly_threader_result** out) {
	return guarded([&]() -> whamd_status_t { return thread_paths(problems, n_problems, device, false, out); });
}

uint64_t whamd_poly_threader_problem_count(const whamd_poly_threader_result* r) { return r ? r->problems.size() : 0; }

uint64_t whamd_poly_threader_position_count(const whamd_poly_threader_result* r, uint64_t m) {
	const auto* p = problem_of(r, m);
	return p ? p->path_cost.size() : 0;
}

uint64_t whamd_poly_threader_section_count(const whamd_poly_threader_result* r, uint64_t m) {
	const auto* p = problem_of(r, m);
	return p ? p->score.size() : 0;
}

uint64_t whamd_poly_threader_cov_count(const whamd_poly_threader_result* r, uint64_t m) {
	const auto* p = problem_of(r, m);
	return p ? p->smoothed.size() : 0;
}

uint64_t whamd_poly_threader_cost_count(const whamd_poly_threader_result* r, uint64_t m) {
	const auto* p = problem_of(r, m);
	return p ? p->all_costs.size() : 0;
}

whamd_status_t whamd_poly_threader_get(const whamd_poly_threader_result* r, uint64_t m, uint32_t* paths_out, float* path_cost_out, uint32_t* smoothed_out,
                                       uint64_t* section_first_out, float* score_out, uint32_t* ambiguous_out, float* all_costs_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	copy_out(paths_out, p->paths);
	copy_out(path_cost_out, p->path_cost);
	copy_out(smoothed_out, p->smoothed);
	copy_out(section_first_out, p->section_first);
	copy_out(score_out, p->score);
	copy_out(ambiguous_out, p->ambiguous);
	copy_out(all_costs_out, p->all_costs);
	return WHAMD_OK;
}

whamd_status_t whamd_poly_threader_get_stats(const whamd_poly_threader_result* r, uint64_t m, whamd_poly_threader_stats* stats_out) {
	return get_stats_of(r, m, stats_out);
}

void whamd_poly_threader_destroy(whamd_poly_threader_result* r) { delete r; }

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_poly_threader_host(const whamd_poly_threader_view* problems, uint64_t n_problems, whamd_poly_threader_result** out) {
	return guarded([&]() -> whamd_status_t { return thread_paths(problems, n_problems, 0, true, out); });
}
#endif

}  // extern "C"
