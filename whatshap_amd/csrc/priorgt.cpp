// priorgt.cpp -- the host side of the prior genotype likelihoods (priorgt.h): validation fused with the mapping of entry positions to
// columns and the packing of (allele, quality) into factor codes, the factor table, result assembly, the C ABI of whatshap_amd.h's prior
// genotypes section; and, in the debug library only, the one-thread host twin (whamd_debug_prior_genotypes_host).
// The mapping is done here and not on the device: the pass over the entries is needed anyway (a read's positions must increase), a
// read's entries lie at neighbouring columns (a step or two forward from the previous one, a binary search only after a gap), and the
// host then knows the number of counted entries exactly -- buffer sizes, and the rule that a call without one launches nothing.
#include "priorgt.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "../../include/whatshap_amd_debug.h"
#include "batch_call.h"
#include "debug_build.h"

using namespace whamd;

namespace {

constexpr uint64_t NONE = std::numeric_limits<uint64_t>::max();
constexpr uint32_t GALLOP = 4;   // linear steps from the previous entry's column before the binary search

// What is wrong with read r, in the order in which the reference's ColumnIterator looks.  `cols`, if given, receives the column of every
// entry (PG_NONE: its position is not in the list).
enum ReadFault { READ_OK = 0, READ_EMPTY, READ_BEFORE_PREVIOUS, READ_NOT_INCREASING, READ_FIRST_NOT_LISTED, READ_LAST_NOT_LISTED };

ReadFault check_read(const whamd_prior_genotypes_view& v, uint64_t r, uint32_t* cols) {
	const uint64_t b = v.read_ptr[r], e = v.read_ptr[r + 1];
	if (b == e) return READ_EMPTY;
	if (r > 0 && v.read_ptr[r - 1] < b && v.entry_position[b] < v.entry_position[v.read_ptr[r - 1]]) return READ_BEFORE_PREVIOUS;
	for (uint64_t x = b + 1; x < e; x++)
		if (v.entry_position[x] <= v.entry_position[x - 1]) return READ_NOT_INCREASING;
	const uint32_t* pos = v.positions;
	const uint64_t n_pos = v.n_positions;
	uint64_t at = std::lower_bound(pos, pos + n_pos, v.entry_position[b]) - pos;
	if (at == n_pos || pos[at] != v.entry_position[b]) return READ_FIRST_NOT_LISTED;
	bool found = true;
	for (uint64_t x = b; x < e; x++) {
		const uint32_t want = v.entry_position[x];
		uint32_t steps = 0;
		while (at < n_pos && pos[at] < want && steps < GALLOP) {
			++at;
			++steps;
		}
		if (at < n_pos && pos[at] < want) at = std::lower_bound(pos + at, pos + n_pos, want) - pos;
		found = at < n_pos && pos[at] == want;
		if (cols) cols[x - b] = found ? (uint32_t)at : PG_NONE;
	}
	return found ? READ_OK : READ_LAST_NOT_LISTED;
}

std::string describe(const whamd_prior_genotypes_view& v, uint64_t r, ReadFault fault) {
	const uint64_t b = v.read_ptr[r], e = v.read_ptr[r + 1];
	const std::string name = "read " + std::to_string(r);
	switch (fault) {
		case READ_EMPTY: return name + " has no entries";
		case READ_BEFORE_PREVIOUS:
			return name + " starts at position " + std::to_string(v.entry_position[b]) + ", before the read in front of it: the reads are not sorted";
		case READ_NOT_INCREASING: return name + ": its positions are not strictly increasing";
		case READ_FIRST_NOT_LISTED: return name + ": its first position " + std::to_string(v.entry_position[b]) + " is not in positions";
		case READ_LAST_NOT_LISTED: return name + ": its last position " + std::to_string(v.entry_position[e - 1]) + " is not in positions";
		default: return name;
	}
}

}  // namespace

void whamd::pg_factor_table(double* table) {
#pragma clang fp contract(off)
	for (uint32_t q = 0; q < PG_QUALITIES; q++) {
		const double p_wrong = std::max(0.05, std::pow(10.0, -((double)q) / 10.0));
		double* ref = table + 3 * q;
		double* alt = table + 3 * (PG_QUALITIES + q);
		ref[0] = 2.0 / 3.0 - 1.0 / 3.0 * p_wrong;
		ref[1] = 1.0 / 3.0;
		ref[2] = 1.0 / 3.0 * p_wrong;
		alt[0] = 1.0 / 3.0 * p_wrong;
		alt[1] = 1.0 / 3.0;
		alt[2] = 2.0 / 3.0 - 1.0 / 3.0 * p_wrong;
	}
}

// ---------------------------------------------------------------------------------------------- validation, mapping, packing
whamd_status_t whamd::priorgt_prepare(const whamd_prior_genotypes_view& v, PriorProblem& p, std::string& msg) {
	if ((v.n_positions && !v.positions) || (v.n_reads && !v.read_ptr)) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (v.want_regularized && (std::isnan(v.constant) || v.constant < 0.0 || std::isnan(v.gt_prob))) {
		msg = "constant is negative or NaN, or gt_prob is NaN";
		return WHAMD_ERR_INVALID;
	}
	if (v.n_reads >= 0xfffff000ull || v.n_positions >= 0xfffff000ull) {
		msg = "2^32 - 4096 or more reads or positions in one problem";
		return WHAMD_ERR_UNSUPPORTED;
	}
	const uint64_t n_reads = v.n_reads, n_pos = v.n_positions;
	for (uint64_t c = 1; c < n_pos; c++)
		if (v.positions[c] <= v.positions[c - 1]) {
			msg = "positions are not strictly increasing: " + std::to_string(v.positions[c]) + " at index " + std::to_string(c) +
			      (v.positions[c] == v.positions[c - 1] ? " is a duplicate" : " comes after a larger one");
			return WHAMD_ERR_INVALID;
		}
	if (!check_offsets(v.read_ptr, n_reads, "read_ptr", "read", msg)) return WHAMD_ERR_INVALID;
	const uint64_t n_entries = n_reads ? v.read_ptr[n_reads] : 0;
	if (n_entries && (!v.entry_position || !v.entry_allele || !v.entry_quality)) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (n_entries >= 0xfffff000ull) {
		msg = "2^32 - 4096 or more entries in one problem";
		return WHAMD_ERR_UNSUPPORTED;
	}
	p.view = &v;
	p.n_reads = n_reads;
	p.n_entries = n_entries;
	p.n_positions = n_pos;
	p.want_reg = v.want_regularized != 0;
	p.column.resize(n_entries);
	p.code.resize(n_entries);

	const uint32_t n_threads = host_threads(n_entries + n_reads, 1 << 16);
	std::vector<uint64_t> bad(n_threads, NONE), counted(n_threads, 0);
	parallel_ranges(n_reads, n_threads, [&](uint64_t rb, uint64_t re, uint32_t t) {
		uint64_t my_bad = NONE, my_counted = 0;
		for (uint64_t r = rb; r < re; r++) {
			const uint64_t b = v.read_ptr[r], e = v.read_ptr[r + 1];
			if (check_read(v, r, p.column.data() + b) != READ_OK) {
				if (my_bad == NONE) my_bad = r;
				continue;
			}
			for (uint64_t x = b; x < e; x++) {
				const uint8_t allele = v.entry_allele[x];
				if (allele > 1) {
					p.column[x] = PG_NONE;
					continue;
				}
				p.code[x] = (uint8_t)(allele * PG_QUALITIES + std::min<uint32_t>(v.entry_quality[x], PG_QUALITIES - 1));
				if (p.column[x] != PG_NONE) ++my_counted;
			}
		}
		bad[t] = my_bad;
		counted[t] = my_counted;
	});
	uint64_t first_bad = NONE;
	for (uint32_t t = 0; t < n_threads; t++) {
		first_bad = std::min(first_bad, bad[t]);
		p.n_counted += counted[t];
	}
	if (first_bad != NONE) {
		msg = describe(v, first_bad, check_read(v, first_bad, nullptr));
		return WHAMD_ERR_INVALID;
	}
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- host twin (debug library)
#ifdef WHAMD_DEBUG_BUILD
namespace {

void priorgt_host(const PriorProblem& p, const double* table, PriorScores& out) {
	const whamd_prior_genotypes_view& v = *p.view;
	const uint64_t n_pos = p.n_positions;
	// the transposition in entry order: count, scan, place -- stable because one thread walks the entries front to back
	out.count.assign(n_pos, 0);
	for (uint64_t x = 0; x < p.n_entries; x++)
		if (p.column[x] != PG_NONE) ++out.count[p.column[x]];
	std::vector<uint64_t> begin(n_pos + 1, 0);
	for (uint64_t c = 0; c < n_pos; c++) begin[c + 1] = begin[c] + out.count[c];
	std::vector<uint8_t> codes(p.n_counted);
	std::vector<uint64_t> cursor(begin.begin(), begin.end() - 1);
	for (uint64_t x = 0; x < p.n_entries; x++)
		if (p.column[x] != PG_NONE) codes[cursor[p.column[x]]++] = p.code[x];
	out.out.resize(n_pos);
	for (uint64_t c = 0; c < n_pos; c++) {
		double d[3];
		pg_chain(codes.data() + begin[c], out.count[c], table, d);
		out.out[c] = pg_tail(d, v.constant, v.gt_prob, p.want_reg);
	}
}

}  // namespace
#endif

// ---------------------------------------------------------------------------------------------- C ABI
struct whamd_prior_genotypes_result {
	struct Problem {
		std::vector<PgOut> out;
		whamd_prior_genotypes_stats stats{};
	};
	std::vector<Problem> problems;
};

namespace {

void assemble(const PriorProblem& p, PriorScores& sc, whamd_prior_genotypes_result::Problem& out) {
	const uint64_t n = p.n_positions;
	whamd_prior_genotypes_stats& s = out.stats;
	s.n_reads = p.n_reads;
	s.n_positions = n;
	s.n_entries = p.n_entries;
	s.n_counted = p.n_counted;
	if (sc.out.empty()) {   // (no counted entry in the problem: every column is the empty chain)
		double table[1] = {0.0}, d[3];
		pg_chain(nullptr, 0, table, d);
		out.out.assign(n, pg_tail(d, p.view->constant, p.view->gt_prob, p.want_reg));
	} else {
		out.out.swap(sc.out);
	}
	for (uint64_t c = 0; c < n; c++) {
		if (out.out[c].genotype >= 0) ++s.n_genotyped;
		const uint32_t k = sc.count.empty() ? 0 : sc.count[c];
		if (!k) continue;
		++s.n_covered;
		++(k <= PG_CLASS_A_MAX ? s.columns_class_a : k <= PG_CLASS_B_MAX ? s.columns_class_b : s.columns_class_c);
		s.longest_run = std::max<uint64_t>(s.longest_run, k);
	}
}

whamd_status_t prior_genotypes(const whamd_prior_genotypes_view* views, uint64_t n, int device, bool host, whamd_prior_genotypes_result** out) {
	BatchClock clock;
	const whamd_status_t st = run_batch<PriorProblem, PriorScores>(
		views, n, host, out, priorgt_prepare,
		[](auto& problems, auto& scores) {
			double table[3 * PG_CODES];
			pg_factor_table(table);
			for (size_t x = 0; x < problems.size(); x++)
				if (problems[x].n_counted) priorgt_host(problems[x], table, scores[x]);
		},
		[&](auto& problems, auto& scores, CallTimes& times, std::string& msg) { return priorgt_device(problems, device, scores, times, msg); }, assemble, &clock);
	if (st != WHAMD_OK) return st;
	for (auto& p : (*out)->problems) p.stats.map_ms = clock.t1 - clock.t0;   // (the mapping is the preparation)
	return WHAMD_OK;
}

}  // namespace

extern "C" {

whamd_status_t whamd_prior_genotypes(const whamd_prior_genotypes_view* problems, uint64_t n_problems, int device, whamd_prior_genotypes_result** out) {
	return guarded([&]() -> whamd_status_t { return prior_genotypes(problems, n_problems, device, false, out); });
}

uint64_t whamd_prior_genotypes_problem_count(const whamd_prior_genotypes_result* r) { return r ? r->problems.size() : 0; }

uint64_t whamd_prior_genotypes_count(const whamd_prior_genotypes_result* r, uint64_t m) { return r && m < r->problems.size() ? r->problems[m].out.size() : 0; }

whamd_status_t whamd_prior_genotypes_get(const whamd_prior_genotypes_result* r, uint64_t m, double* gl_out, int8_t* genotype_out, double* reg_out,
                                         int8_t* reg_genotype_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	const std::vector<PgOut>& o = p->out;
	for (size_t c = 0; c < o.size(); c++) {
		if (gl_out) std::memcpy(gl_out + 3 * c, o[c].gl, sizeof o[c].gl);
		if (genotype_out) genotype_out[c] = (int8_t)o[c].genotype;
		if (reg_out) std::memcpy(reg_out + 3 * c, o[c].reg, sizeof o[c].reg);
		if (reg_genotype_out) reg_genotype_out[c] = (int8_t)o[c].reg_genotype;
	}
	return WHAMD_OK;
}

whamd_status_t whamd_prior_genotypes_get_stats(const whamd_prior_genotypes_result* r, uint64_t m, whamd_prior_genotypes_stats* stats_out) {
	return get_stats_of(r, m, stats_out);
}

void whamd_prior_genotypes_destroy(whamd_prior_genotypes_result* r) { delete r; }

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_prior_genotypes_host(const whamd_prior_genotypes_view* problems, uint64_t n_problems, whamd_prior_genotypes_result** out) {
	return guarded([&]() -> whamd_status_t { return prior_genotypes(problems, n_problems, 0, true, out); });
}
#endif

}  // extern "C"
