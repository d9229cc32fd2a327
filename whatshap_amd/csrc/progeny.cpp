// progeny.cpp -- the host side of progeny marker scoring (progeny.h): validation, the weight vectors and stride list, the entry list
// with the row each stored entry really reads, the validation of depth problems (genotype likelihoods from allele depths), the C ABI of whatshap_amd.h's progeny section; and, in the debug library only, the
// one-thread host twins (whamd_debug_progeny_*).
#include "progeny.h"

#include <algorithm>
#include <cstring>
#include <limits>
#include <memory>

#include "../../include/whatshap_amd_debug.h"
#include "batch_call.h"
#include "debug_build.h"

using namespace whamd;

namespace {

constexpr uint64_t NO_ERROR = std::numeric_limits<uint64_t>::max();

// The walk of one anchor over its partners in stride order (offspringscoring.py:156-186).  emit(j, kind, eff, reused) for every stored
// entry; returns the first partner whose type has no score kind, or NO_ERROR.
template <class Emit>
uint64_t walk_anchor(const whamd_progeny_view& v, const std::vector<uint32_t>& strides, uint64_t i, Emit&& emit) {
	const uint32_t ni = v.node_variant[i];
	const bool anchor_sn = v.alt_count[ni] == 1 && v.co_alt_count[ni] == 0;
	int64_t prev_variant = -1;
	uint32_t prev_eff = 0;
	uint8_t prev_kind = 0;
	for (const uint32_t s : strides) {
		const uint64_t j = i + s;
		if (j >= v.n_nodes) break;   // the strides increase
		const uint32_t nj = v.node_variant[j];
		if (nj == ni) {
			emit(j, (uint8_t)PROGENY_KIND_INF, (uint32_t)j, false);
			continue;
		}
		if (!anchor_sn) continue;
		if ((int64_t)nj == prev_variant) {
			emit(j, prev_kind, prev_eff, true);
			continue;
		}
		const uint32_t alt = v.alt_count[nj], co = v.co_alt_count[nj];
		uint8_t kind;
		if (alt == 1 && co == 0) kind = PROGENY_KIND_SN;
		else if (alt == 2 && co == 0) kind = PROGENY_KIND_DN;
		else if (alt == 1 && co == 1) kind = PROGENY_KIND_S2;
		else return j;
		prev_variant = nj;
		prev_eff = (uint32_t)j;
		prev_kind = kind;
		emit(j, kind, (uint32_t)j, false);
	}
	return NO_ERROR;
}

whamd_status_t validate(const whamd_progeny_view& v, std::string& msg, bool needs_table = true) {
	if (v.ploidy < 2) {
		msg = "ploidy " + std::to_string(v.ploidy) + " below 2: the reference's start value is log(1 / (ploidy - 1))";
		return WHAMD_ERR_INVALID;
	}
	if (v.scoring_window < 1) {
		msg = "scoring_window must be at least 1";
		return WHAMD_ERR_INVALID;
	}
	if (v.scoring_window < 4) {
		msg = "scoring_window " + std::to_string(v.scoring_window) + " below 4: the reference's stride list is undefined there (it raises IndexError)";
		return WHAMD_ERR_INVALID;
	}
	if (needs_table && v.n_samples && v.n_positions && !v.gl) {
		msg = "null table";
		return WHAMD_ERR_INVALID;
	}
	if ((v.n_nodes && !v.node_variant) || (v.n_variants && (!v.alt_count || !v.co_alt_count))) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	// getIndex is uint32 arithmetic, and the constructor sizes the vector for numPositions + 1 rows
	const long double cells = ((long double)v.n_positions + 1) * v.n_samples * ((long double)v.ploidy + 1);
	if (cells >= 4294967296.0L) {
		msg = "(n_positions + 1) * n_samples * (ploidy + 1) reaches 2^32: the reference's uint32 index would wrap";
		return WHAMD_ERR_INVALID;
	}
	if (v.n_nodes >= 0xffffffffull) {
		msg = "more than 2^32 - 2 nodes";
		return WHAMD_ERR_INVALID;
	}
	for (uint64_t x = 0; x < v.n_nodes; x++) {
		if (v.node_variant[x] >= v.n_variants) {
			msg = "node " + std::to_string(x) + " names variant " + std::to_string(v.node_variant[x]) + ", but only " + std::to_string(v.n_variants) +
			      " variant types were given (mismatched lengths)";
			return WHAMD_ERR_INVALID;
		}
	}
	return WHAMD_OK;
}

std::string type_error(const whamd_progeny_view& v, uint64_t i, uint64_t j) {
	const uint32_t nj = v.node_variant[j];
	return "pair (" + std::to_string(i) + ", " + std::to_string(j) + "): variant " + std::to_string(nj) + " has (alt_count, co_alt_count) = (" +
	       std::to_string(v.alt_count[nj]) + ", " + std::to_string(v.co_alt_count[nj]) + "), which has no score kind (only (1, 0), (2, 0) and (1, 1) have)";
}

}  // namespace

// ---------------------------------------------------------------------------------------------- weights, strides
void whamd::progeny_weights(uint32_t ploidy, ProgenyWeights& w) {
	const double k = (double)ploidy;
	double* sn = w.same[PROGENY_KIND_SN];
	double* dn = w.diff[PROGENY_KIND_SN];
	sn[0] = 0.5; sn[1] = 0; sn[2] = 0; sn[3] = 0.5; sn[4] = 0; sn[5] = 0;
	dn[0] = (k / 2 - 1) / (2 * (k - 1));
	dn[1] = k / (4 * (k - 1));
	dn[2] = k / (4 * (k - 1));
	dn[3] = (k / 2 - 1) / (2 * (k - 1));
	dn[4] = 0;
	dn[5] = 0;
	double* s2 = w.same[PROGENY_KIND_S2];
	double* d2 = w.diff[PROGENY_KIND_S2];
	s2[0] = sn[0] / 2.0;
	s2[1] = sn[1] / 2.0;
	d2[0] = dn[0] / 2.0;
	d2[1] = dn[1] / 2.0;
	for (int c = 2; c < 6; c++) {
		s2[c] = (sn[c] + sn[c - 2]) / 2.0;
		d2[c] = (dn[c] + dn[c - 2]) / 2.0;
	}
	double* sd = w.same[PROGENY_KIND_DN];
	double* dd = w.diff[PROGENY_KIND_DN];
	sd[0] = (k / 2 - 1) / (2 * (k - 1));
	sd[1] = 0;
	sd[2] = k / (4 * (k - 1));
	sd[3] = k / (4 * (k - 1));
	sd[4] = 0;
	sd[5] = (k / 2 - 1) / (2 * (k - 1));
	dd[0] = (k / 2 - 2) * (k / 2 - 1) / (2 * (k - 1) * (k - 2));
	dd[1] = (k / 2) * (k / 2 - 1) / (2 * (k - 1) * (k - 2));
	dd[2] = (k / 2) * (k / 2 - 1) / (k - 1) * (k - 2);   // (the reference's expression: divided by k - 1, then multiplied by k - 2)
	dd[3] = (k / 2) * (k / 2 - 1) / (k - 1) * (k - 2);
	dd[4] = (k / 2) * (k / 2 - 1) / (2 * (k - 1) * (k - 2));
	dd[5] = (k / 2 - 2) * (k / 2 - 1) / (2 * (k - 1) * (k - 2));
	w.start = std::log(1.0 / (double)(ploidy - 1));
}

std::vector<uint32_t> whamd::progeny_strides(uint32_t w) {
	const uint32_t w3 = w / 4, w7 = w / 2, w13 = (uint32_t)(3 * (uint64_t)w / 4);
	std::vector<uint32_t> s;
	for (uint32_t i = 1; i <= w3; i++) s.push_back(i);
	uint32_t last = s.empty() ? 0 : s.back();   // (w >= 4: never empty)
	for (uint32_t i = 1; i <= w7 - w3; i++) s.push_back(last + 3 * i);
	last = s.empty() ? 0 : s.back();
	for (uint32_t i = 1; i <= w13 - w7; i++) s.push_back(last + 7 * i);
	last = s.empty() ? 0 : s.back();
	for (uint32_t i = 1; i <= w - w13; i++) s.push_back(last + 13 * i);
	return s;
}

// ---------------------------------------------------------------------------------------------- the entry list
whamd_status_t whamd::progeny_prepare(const whamd_progeny_view& v, ProgenyProblem& p, std::string& msg, bool needs_table) {
	const whamd_status_t st = validate(v, msg, needs_table);
	if (st != WHAMD_OK) return st;
	p.gl = v.gl;
	p.n_positions = v.n_positions;
	p.n_nodes = v.n_nodes;
	p.n_samples = v.n_samples;
	p.ploidy = v.ploidy;
	progeny_weights(v.ploidy, p.w);
	const std::vector<uint32_t> strides = progeny_strides(v.scoring_window);
	const uint64_t n = v.n_nodes, reach = strides.back();
	if (!n) return WHAMD_OK;
	// Entries go out in triangular order: by partner hi = j, then by anchor lo = i.  Ranges of hi are independent: the range [b, e) hears from
	// the anchors b - reach .. e - 1, walked in increasing order, so every hi's entries arrive sorted by anchor.  Two passes: count, fill.
	std::vector<uint64_t> first(n + 1, 0);
	const uint32_t n_threads = host_threads(n * strides.size(), 1 << 18);
	const uint64_t n_ranges = std::min<uint64_t>(n, (uint64_t)n_threads * 4);
	std::vector<uint64_t> bad_i(n_ranges, NO_ERROR), bad_j(n_ranges, NO_ERROR), inf_of(n_ranges, 0), reused_of(n_ranges, 0);
	auto range = [&](uint64_t r, uint64_t& b, uint64_t& e) {
		b = n * r / n_ranges;
		e = n * (r + 1) / n_ranges;
	};
	parallel_ranges(n_ranges, n_threads, [&](uint64_t rb, uint64_t re, uint32_t) {
		for (uint64_t r = rb; r < re; r++) {
			uint64_t b, e;
			range(r, b, e);
			for (uint64_t i = b > reach ? b - reach : 0; i < e; i++) {
				const uint64_t bad = walk_anchor(v, strides, i, [&](uint64_t j, uint8_t kind, uint32_t, bool reused) {
					if (j < b || j >= e) return;
					++first[j + 1];
					if (kind == PROGENY_KIND_INF) ++inf_of[r];
					if (reused) ++reused_of[r];
				});
				if (bad != NO_ERROR && bad_i[r] == NO_ERROR) {
					bad_i[r] = i;
					bad_j[r] = bad;
				}
			}
		}
	});
	uint64_t worst = NO_ERROR;
	for (uint64_t r = 0; r < n_ranges; r++) {
		if (bad_i[r] != NO_ERROR && (worst == NO_ERROR || bad_i[r] < bad_i[worst])) worst = r;
		p.n_inf += inf_of[r];
		p.n_reused += reused_of[r];
	}
	if (worst != NO_ERROR) {
		msg = type_error(v, bad_i[worst], bad_j[worst]);
		return WHAMD_ERR_INVALID;
	}
	for (uint64_t j = 0; j < n; j++) first[j + 1] += first[j];
	const uint64_t total = first[n];
	p.lo.resize(total);
	p.hi.resize(total);
	p.eff.resize(total);
	p.kind.resize(total);
	parallel_ranges(n_ranges, n_threads, [&](uint64_t rb, uint64_t re, uint32_t) {
		for (uint64_t r = rb; r < re; r++) {
			uint64_t b, e;
			range(r, b, e);
			std::vector<uint64_t> cursor(first.begin() + b, first.begin() + e);
			for (uint64_t i = b > reach ? b - reach : 0; i < e; i++) {
				walk_anchor(v, strides, i, [&](uint64_t j, uint8_t kind, uint32_t eff, bool) {
					if (j < b || j >= e) return;
					const uint64_t x = cursor[j - b]++;
					p.lo[x] = (uint32_t)i;
					p.hi[x] = (uint32_t)j;
					p.eff[x] = eff;
					p.kind[x] = kind;
				});
			}
		}
	});
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- depth problems
whamd_status_t whamd::progeny_depths_prepare(const whamd_progeny_depths_view& v, ProgenyDepths& d, std::string& msg) {
	if (v.ploidy < 2) {
		msg = "ploidy " + std::to_string(v.ploidy) + " below 2";
		return WHAMD_ERR_INVALID;
	}
	if (!(v.error_rate > 0.0 && v.error_rate < 1.0)) {
		msg = "error_rate " + std::to_string(v.error_rate) + " outside (0, 1)";
		return WHAMD_ERR_INVALID;
	}
	if ((v.n_rows && v.n_samples && (!v.ref_depth || !v.alt_depth)) || (v.n_nodes && !v.node_row) ||
	    (v.priors && v.n_rows && (!v.row_alt_count || !v.row_co_alt_count))) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	// the table has n_nodes rows: the guard of the score call (getIndex is uint32 arithmetic, the constructor sizes for one row more)
	const long double cells = ((long double)v.n_nodes + 1) * v.n_samples * ((long double)v.ploidy + 1);
	if (cells >= 4294967296.0L) {
		msg = "(n_nodes + 1) * n_samples * (ploidy + 1) reaches 2^32: the reference's uint32 index would wrap";
		return WHAMD_ERR_INVALID;
	}
	if (v.n_rows >= 0xffffffffull) {
		msg = "more than 2^32 - 2 depth rows";
		return WHAMD_ERR_INVALID;
	}
	for (uint64_t x = 0; x < v.n_nodes; x++) {
		if (v.node_row[x] >= v.n_rows) {
			msg = "node " + std::to_string(x) + " names depth row " + std::to_string(v.node_row[x]) + ", but only " + std::to_string(v.n_rows) + " rows were given";
			return WHAMD_ERR_INVALID;
		}
	}
	d.ref = v.ref_depth;
	d.alt = v.alt_depth;
	d.n_rows = v.n_rows;
	d.n_nodes = v.n_nodes;
	d.n_samples = v.n_samples;
	d.ploidy = v.ploidy;
	d.error_rate = v.error_rate;
	d.node_row = v.node_row;
	d.priors = v.priors;
	d.row_prior.clear();
	if (v.priors) {
		const uint64_t k1 = (uint64_t)v.ploidy + 1;
		d.row_prior.resize(v.n_rows);
		for (uint64_t r = 0; r < v.n_rows; r++) {
			const uint32_t alt = v.row_alt_count[r], co = v.row_co_alt_count[r];
			if (alt > v.ploidy || co > v.ploidy) {
				msg = "depth row " + std::to_string(r) + " has (alt_count, co_alt_count) = (" + std::to_string(alt) + ", " + std::to_string(co) +
				      "), above the ploidy " + std::to_string(v.ploidy) + ": the priors have no such row";
				return WHAMD_ERR_INVALID;
			}
			const uint64_t first = (alt * k1 + co) * k1;
			bool positive = false, bad = false;
			for (uint64_t g = 0; g < k1; g++) {
				const double p = v.priors[first + g];
				bad = bad || !(p >= 0.0) || std::isinf(p);
				positive = positive || p > 0.0;
			}
			if (bad || !positive) {
				msg = "priors[" + std::to_string(alt) + "][" + std::to_string(co) + "] (depth row " + std::to_string(r) +
				      ") is negative, not finite or all zero: the likelihoods cannot be normalised";
				return WHAMD_ERR_INVALID;
			}
			d.row_prior[r] = (uint32_t)first;
		}
	}
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- host twins (debug library)
#ifdef WHAMD_DEBUG_BUILD
namespace {

double entry_score_host(const ProgenyProblem& p, uint32_t lo, uint32_t eff, uint8_t kind, const float* zero_row) {
	if (kind == PROGENY_KIND_INF) return -std::numeric_limits<double>::infinity();
	return progeny_pair_score(progeny_row(p, lo, zero_row), progeny_row(p, eff, zero_row), p.ploidy + 1, 1, p.n_samples, p.w.same[kind], p.w.diff[kind],
	                          kind == PROGENY_KIND_SN ? 4 : 6, p.w.start);
}

void progeny_score_host(const ProgenyProblem& p, ProgenyResult& out) {
	const std::vector<float> zero_row((size_t)p.n_samples * (p.ploidy + 1), 0.0f);
	out.score.resize(p.lo.size());
	for (size_t x = 0; x < p.lo.size(); x++) out.score[x] = entry_score_host(p, p.lo[x], p.eff[x], p.kind[x], zero_row.data());
}

// progeny_gl_kernel's loop on one thread: the same cell function on the caller's arrays.
void progeny_gl_host(const ProgenyDepths& d, float* table, double* table_f64) {
	const uint64_t k1 = (uint64_t)d.ploidy + 1;
	for (uint64_t node = 0; node < d.n_nodes; node++) {
		const uint32_t row = d.node_row[node];
		for (uint64_t s = 0; s < d.n_samples; s++) {
			const uint64_t w = s * d.n_rows + row, v = (node * d.n_samples + s) * k1;
			progeny_gl_cell(d.ref[w], d.alt[w], d.ploidy, d.error_rate, d.priors ? d.priors + d.row_prior[row] : nullptr, nullptr, 0,
			                table ? table + v : nullptr, table_f64 ? table_f64 + v : nullptr);
		}
	}
}

}  // namespace
#endif

// ---------------------------------------------------------------------------------------------- C ABI
struct whamd_progeny_scores {
	std::vector<ProgenyProblem> problems;
	std::vector<ProgenyResult> results;
	std::vector<whamd_progeny_score_stats> stats;
};

namespace {

// Counts and times of a finished call into its stats.
void fill_stats(whamd_progeny_scores& r, const CallTimes& times, BatchClock clock) {
	clock.t2 = clock.t3 = now_ms();   // (nothing is assembled: the results are the scores)
	for (size_t x = 0; x < r.problems.size(); x++) {
		const ProgenyProblem& p = r.problems[x];
		whamd_progeny_score_stats& s = r.stats[x];
		s.n_nodes = p.n_nodes;
		s.n_entries = p.lo.size();
		s.n_inf = p.n_inf;
		s.n_reused = p.n_reused;
		s.n_sample_terms = (p.lo.size() - p.n_inf) * (uint64_t)p.n_samples;
		stamp_times(s, times, clock);
	}
}

whamd_status_t score(const whamd_progeny_view* views, uint64_t n, int device, bool host, whamd_progeny_scores** out) {
	if (!out || (n && !views)) return fail(WHAMD_ERR_INVALID, "null argument");
	*out = nullptr;
	BatchClock clock;
	clock.t0 = now_ms();
	std::unique_ptr<whamd_progeny_scores> r(new whamd_progeny_scores());
	r->problems.resize(n);
	r->results.resize(n);
	r->stats.assign(n, whamd_progeny_score_stats{});
	std::string msg;
	for (uint64_t x = 0; x < n; x++) {
		const whamd_status_t st = progeny_prepare(views[x], r->problems[x], msg);
		if (st != WHAMD_OK) return fail(st, n > 1 ? "problem " + std::to_string(x) + ": " + msg : msg);
	}
	clock.t1 = now_ms();
	CallTimes times;
	if (host) {
#ifdef WHAMD_DEBUG_BUILD
		for (uint64_t x = 0; x < n; x++) progeny_score_host(r->problems[x], r->results[x]);
#endif
	} else {
		const whamd_status_t st = progeny_score_device(r->problems, device, r->results, times, msg);
		if (st != WHAMD_OK) return fail(st, msg);
	}
	fill_stats(*r, times, clock);
	*out = r.release();
	return WHAMD_OK;
}

whamd_status_t prepare_depths(const whamd_progeny_depths_view* views, uint64_t n, std::vector<ProgenyDepths>& ds, std::string& msg) {
	ds.resize(n);
	for (uint64_t x = 0; x < n; x++) {
		const whamd_status_t st = progeny_depths_prepare(views[x], ds[x], msg);
		if (st != WHAMD_OK) {
			if (n > 1) msg = "problem " + std::to_string(x) + ": " + msg;
			return st;
		}
	}
	return WHAMD_OK;
}

whamd_status_t gl(const whamd_progeny_depths_view* views, uint64_t n, int device, bool host, float* const* table_out, double* const* table_f64_out) {
	if (n && !views) return fail(WHAMD_ERR_INVALID, "null argument");
	std::vector<ProgenyDepths> ds;
	std::string msg;
	whamd_status_t st = prepare_depths(views, n, ds, msg);
	if (st != WHAMD_OK) return fail(st, msg);
	if (host) {
#ifdef WHAMD_DEBUG_BUILD
		for (uint64_t x = 0; x < n; x++) progeny_gl_host(ds[x], table_out ? table_out[x] : nullptr, table_f64_out ? table_f64_out[x] : nullptr);
#endif
		return WHAMD_OK;
	}
	st = progeny_gl_device(ds, device, table_out, table_f64_out, msg);
	return st == WHAMD_OK ? st : fail(st, msg);
}

whamd_status_t score_depths(const whamd_progeny_depths_view* views, uint64_t n, int device, whamd_progeny_scores** out) {
	if (!out || (n && !views)) return fail(WHAMD_ERR_INVALID, "null argument");
	*out = nullptr;
	BatchClock clock;
	clock.t0 = now_ms();
	std::unique_ptr<whamd_progeny_scores> r(new whamd_progeny_scores());
	r->problems.resize(n);
	r->results.resize(n);
	r->stats.assign(n, whamd_progeny_score_stats{});
	std::vector<ProgenyDepths> ds;
	std::string msg;
	whamd_status_t st = prepare_depths(views, n, ds, msg);
	if (st != WHAMD_OK) return fail(st, msg);
	for (uint64_t x = 0; x < n; x++) {
		const whamd_progeny_depths_view& v = views[x];
		// the table the device makes has one row per node
		const whamd_progeny_view pv{nullptr, v.n_nodes, v.n_samples, v.ploidy, v.n_nodes, v.node_variant, v.n_variants, v.alt_count, v.co_alt_count, v.scoring_window};
		st = progeny_prepare(pv, r->problems[x], msg, false);
		if (st != WHAMD_OK) return fail(st, n > 1 ? "problem " + std::to_string(x) + ": " + msg : msg);
	}
	clock.t1 = now_ms();
	CallTimes times;
	st = progeny_score_depths_device(ds, r->problems, device, r->results, times, msg);
	if (st != WHAMD_OK) return fail(st, msg);
	fill_stats(*r, times, clock);
	*out = r.release();
	return WHAMD_OK;
}

struct TypesArgs {
	const float* gl;
	uint64_t n_positions;
	uint32_t n_samples, ploidy;
	const double* priors;
	const uint32_t* nodes;
	uint64_t n_nodes;
};

whamd_status_t variant_types(const TypesArgs& a, int device, bool host, double* llh_out, uint32_t* g0_out, uint32_t* g1_out) {
	if (!a.priors || (a.n_nodes && !llh_out) || (a.n_samples && a.n_positions && !a.gl)) return fail(WHAMD_ERR_INVALID, "null argument");
	if (a.ploidy < 1 || a.ploidy > 64) return fail(WHAMD_ERR_INVALID, "ploidy " + std::to_string(a.ploidy) + " outside 1 .. 64");
	const long double cells = ((long double)a.n_positions + 1) * a.n_samples * ((long double)a.ploidy + 1);
	if (cells >= 4294967296.0L) return fail(WHAMD_ERR_INVALID, "(n_positions + 1) * n_samples * (ploidy + 1) reaches 2^32: the reference's uint32 index would wrap");
	const uint32_t k1 = a.ploidy + 1, n_types = k1 * (k1 + 1) / 2;
	const uint64_t n = a.n_nodes, row = (uint64_t)a.n_samples * k1;
	if (!n) return WHAMD_OK;
	// the priors of the types in loop order (g0, g1 <= g0), the rows of the asked nodes (zeros beyond n_positions: getGl returns 0.0 there)
	std::vector<double> prior((size_t)n_types * k1);
	uint32_t t = 0;
	for (uint32_t g0 = 0; g0 < k1; g0++)
		for (uint32_t g1 = 0; g1 <= g0; g1++, t++) std::memcpy(&prior[(size_t)t * k1], a.priors + ((size_t)g0 * k1 + g1) * k1, k1 * sizeof(double));
	RawVec<float> rows(n * row);
	for (uint64_t x = 0; x < n; x++) {
		const uint64_t node = a.nodes ? a.nodes[x] : x;
		if (node < a.n_positions) std::memcpy(rows.data() + x * row, a.gl + node * row, row * sizeof(float));
		else std::fill(rows.begin() + x * row, rows.begin() + (x + 1) * row, 0.0f);
	}
	if (host) {
#ifdef WHAMD_DEBUG_BUILD
		for (uint64_t x = 0; x < n; x++)
			for (uint32_t ty = 0; ty < n_types; ty++) llh_out[x * n_types + ty] = progeny_type_llh(rows.data() + x * row, a.n_samples, k1, &prior[(size_t)ty * k1]);
#endif
	} else if (a.n_samples == 0) {
		std::fill(llh_out, llh_out + n * n_types, 1.0);   // nothing to sum: the start value, no device work
	} else {
		std::string msg;
		const whamd_status_t st = progeny_types_device(rows.data(), n, a.n_samples, k1, prior.data(), device, llh_out, msg);
		if (st != WHAMD_OK) return fail(st, msg);
	}
	// the first type, in loop order, with a strictly larger llh
	for (uint64_t x = 0; x < n; x++) {
		uint32_t best0 = 0, best1 = 0;
		double best = -std::numeric_limits<double>::infinity();
		uint32_t ty = 0;
		for (uint32_t g0 = 0; g0 < k1; g0++)
			for (uint32_t g1 = 0; g1 <= g0; g1++, ty++)
				if (llh_out[x * n_types + ty] > best) {
					best = llh_out[x * n_types + ty];
					best0 = g0;
					best1 = g1;
				}
		if (g0_out) g0_out[x] = best0;
		if (g1_out) g1_out[x] = best1;
	}
	return WHAMD_OK;
}

}  // namespace

extern "C" {

whamd_status_t whamd_progeny_score(const whamd_progeny_view* problems, uint64_t n_problems, int device, whamd_progeny_scores** out) {
	return guarded([&]() -> whamd_status_t { return score(problems, n_problems, device, false, out); });
}

uint64_t whamd_progeny_score_problem_count(const whamd_progeny_scores* s) { return s ? s->results.size() : 0; }

uint64_t whamd_progeny_score_count(const whamd_progeny_scores* s, uint64_t m) { return s && m < s->problems.size() ? s->problems[m].lo.size() : 0; }

whamd_status_t whamd_progeny_score_get(const whamd_progeny_scores* s, uint64_t m, uint32_t* i_out, uint32_t* j_out, float* score_f32_out,
                                       double* score_f64_out) {
	return guarded([&]() -> whamd_status_t {
		if (!s) return fail(WHAMD_ERR_INVALID, "null argument");
		if (m >= s->problems.size()) return fail(WHAMD_ERR_INVALID, "problem index out of range");
		const ProgenyProblem& p = s->problems[m];
		const ProgenyResult& r = s->results[m];
		const size_t n = r.score.size();
		if (i_out) progeny_copy(i_out, p.hi.data(), n * 4);
		if (j_out) progeny_copy(j_out, p.lo.data(), n * 4);
		if (score_f32_out)   // TriangleSparseMatrix.set: the double rounded to float
			parallel_ranges(n, host_threads(n, 1 << 20), [&](uint64_t b, uint64_t e, uint32_t) {
				for (uint64_t x = b; x < e; x++) score_f32_out[x] = (float)r.score[x];
			});
		if (score_f64_out) progeny_copy(score_f64_out, r.score.data(), n * 8);
		return WHAMD_OK;
	});
}

whamd_status_t whamd_progeny_score_get_stats(const whamd_progeny_scores* s, uint64_t m, whamd_progeny_score_stats* stats_out) {
	if (!s || !stats_out) return fail(WHAMD_ERR_INVALID, "null argument");
	if (m >= s->stats.size()) return fail(WHAMD_ERR_INVALID, "problem index out of range");
	*stats_out = s->stats[m];
	return WHAMD_OK;
}

void whamd_progeny_score_destroy(whamd_progeny_scores* s) { delete s; }

whamd_status_t whamd_progeny_variant_types(const float* gl, uint64_t n_positions, uint32_t n_samples, uint32_t ploidy, const double* priors,
                                           const uint32_t* nodes, uint64_t n_nodes, int device, double* llh_out, uint32_t* g0_out, uint32_t* g1_out) {
	return guarded([&]() -> whamd_status_t {
		return variant_types(TypesArgs{gl, n_positions, n_samples, ploidy, priors, nodes, n_nodes}, device, false, llh_out, g0_out, g1_out);
	});
}

whamd_status_t whamd_progeny_gl(const whamd_progeny_depths_view* problems, uint64_t n_problems, int device, float* const* table_out,
                                double* const* table_f64_out) {
	return guarded([&]() -> whamd_status_t { return gl(problems, n_problems, device, false, table_out, table_f64_out); });
}

whamd_status_t whamd_progeny_score_depths(const whamd_progeny_depths_view* problems, uint64_t n_problems, int device, whamd_progeny_scores** out) {
	return guarded([&]() -> whamd_status_t { return score_depths(problems, n_problems, device, out); });
}

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_progeny_gl_host(const whamd_progeny_depths_view* problems, uint64_t n_problems, float* const* table_out,
                                           double* const* table_f64_out) {
	return guarded([&]() -> whamd_status_t { return gl(problems, n_problems, 0, true, table_out, table_f64_out); });
}

whamd_status_t whamd_debug_progeny_score_host(const whamd_progeny_view* problems, uint64_t n_problems, whamd_progeny_scores** out) {
	return guarded([&]() -> whamd_status_t { return score(problems, n_problems, 0, true, out); });
}

whamd_status_t whamd_debug_progeny_score_entries_host(const whamd_progeny_view* problem, uint64_t n_entries, const uint32_t* i, const uint32_t* j,
                                                      double* score_out, uint8_t* stored_out) {
	return guarded([&]() -> whamd_status_t {
		if (!problem || (n_entries && (!i || !j || !score_out || !stored_out))) return fail(WHAMD_ERR_INVALID, "null argument");
		std::string msg;
		const whamd_status_t st = validate(*problem, msg);
		if (st != WHAMD_OK) return fail(st, msg);
		ProgenyProblem p;
		p.gl = problem->gl;
		p.n_positions = problem->n_positions;
		p.n_nodes = problem->n_nodes;
		p.n_samples = problem->n_samples;
		p.ploidy = problem->ploidy;
		progeny_weights(p.ploidy, p.w);
		const std::vector<uint32_t> strides = progeny_strides(problem->scoring_window);
		const std::vector<float> zero_row((size_t)p.n_samples * (p.ploidy + 1), 0.0f);
		for (uint64_t x = 0; x < n_entries; x++) {
			const uint32_t lo = std::min(i[x], j[x]), hi = std::max(i[x], j[x]);
			stored_out[x] = 0;
			score_out[x] = 0.0;
			if (hi >= p.n_nodes) continue;
			const uint64_t bad = walk_anchor(*problem, strides, lo, [&](uint64_t jj, uint8_t kind, uint32_t eff, bool) {
				if (jj != hi) return;
				stored_out[x] = 1;
				score_out[x] = entry_score_host(p, lo, eff, kind, zero_row.data());
			});
			if (bad != NO_ERROR && bad <= hi) return fail(WHAMD_ERR_INVALID, type_error(*problem, lo, bad));
		}
		return WHAMD_OK;
	});
}

whamd_status_t whamd_debug_progeny_pair_score_host(const float* gl, uint64_t n_positions, uint32_t n_samples, uint32_t ploidy, uint64_t pos1,
                                                   uint64_t pos2, uint32_t kind, double* score_out) {
	return guarded([&]() -> whamd_status_t {
		if (!score_out || (n_samples && n_positions && !gl)) return fail(WHAMD_ERR_INVALID, "null argument");
		if (ploidy < 2) return fail(WHAMD_ERR_INVALID, "ploidy " + std::to_string(ploidy) + " below 2: the reference's start value is log(1 / (ploidy - 1))");
		if (kind > PROGENY_KIND_DN) return fail(WHAMD_ERR_INVALID, "score kind outside 0 .. 2");
		ProgenyProblem p;
		p.gl = gl;
		p.n_positions = n_positions;
		p.n_samples = n_samples;
		p.ploidy = ploidy;
		progeny_weights(ploidy, p.w);
		const std::vector<float> zero_row((size_t)n_samples * (ploidy + 1), 0.0f);
		*score_out = progeny_pair_score(progeny_row(p, pos1, zero_row.data()), progeny_row(p, pos2, zero_row.data()), ploidy + 1, 1, n_samples, p.w.same[kind],
		                                p.w.diff[kind], kind == PROGENY_KIND_SN ? 4 : 6, p.w.start);
		return WHAMD_OK;
	});
}

whamd_status_t whamd_debug_progeny_variant_types_host(const float* gl, uint64_t n_positions, uint32_t n_samples, uint32_t ploidy, const double* priors,
                                                      const uint32_t* nodes, uint64_t n_nodes, double* llh_out, uint32_t* g0_out, uint32_t* g1_out) {
	return guarded([&]() -> whamd_status_t {
		return variant_types(TypesArgs{gl, n_positions, n_samples, ploidy, priors, nodes, n_nodes}, 0, true, llh_out, g0_out, g1_out);
	});
}
#endif

}  // extern "C"
