// tagphase.cpp -- the host side of haplotagphase (tagphase.h): validation, phase sets to dense ids (per read), result assembly, the C ABI of
// whatshap_amd.h's haplotagphase section; and, in the debug library only, the one-thread host twin of the voting (whamd_debug_tagphase_host).
// The only pass over the entries here is the validation: bounds of every entry, the number of voting entries and the sum of their
// magnitudes (the 2^53 rule) -- independent per entry, so it could move to the device.
#include "tagphase.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <unordered_map>

#include "../../include/whatshap_amd_debug.h"
#include "batch_call.h"
#include "debug_build.h"

using namespace whamd;

namespace {

constexpr uint64_t NONE = std::numeric_limits<uint64_t>::max();

}  // namespace

// ---------------------------------------------------------------------------------------------- validation, phase sets
whamd_status_t whamd::tagphase_prepare(const whamd_tagphase_view& v, TagphaseProblem& p, std::string& msg) {
	if ((v.n_variants && !v.variant_flags) || (v.n_reads && (!v.read_ptr || !v.read_ps || !v.read_hp))) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (std::isnan(v.gap_threshold)) {
		msg = "gap_threshold is NaN";
		return WHAMD_ERR_INVALID;
	}
	if (v.n_reads >= 0xffffffffull || v.n_variants >= 0xffffffffull) {
		msg = "2^32 - 1 or more reads or variants in one problem";
		return WHAMD_ERR_UNSUPPORTED;
	}
	const uint64_t n_reads = v.n_reads, n_var = v.n_variants;
	if (!check_offsets(v.read_ptr, n_reads, "read_ptr", "read", msg)) return WHAMD_ERR_INVALID;
	const uint64_t n_entries = n_reads ? v.read_ptr[n_reads] : 0;
	if (n_entries && (!v.entry_variant || !v.entry_id || !v.entry_quality)) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (n_entries >= 0xffffffffull) {
		msg = "2^32 - 1 or more entries in one problem";
		return WHAMD_ERR_UNSUPPORTED;
	}
	for (uint64_t x = 0; x < n_var; x++)
		if (v.variant_flags[x] > (WHAMD_TAGPHASE_HOMOZYGOUS | WHAMD_TAGPHASE_PHASED | WHAMD_TAGPHASE_SNV)) {
			msg = "variant " + std::to_string(x) + ": flags " + std::to_string((int)v.variant_flags[x]) + " have bits above bit 2";
			return WHAMD_ERR_INVALID;
		}
	p.view = &v;
	p.n_reads = n_reads;
	p.n_entries = n_entries;
	p.n_variants = n_var;
	p.want_table = v.want_table != 0;

	// per read: does it vote, and for which phase set
	p.read_code.assign(n_reads, TP_NOT_COUNTED);
	std::unordered_map<int64_t, uint32_t> ps_id;
	for (uint64_t r = 0; r < n_reads; r++) {
		const int64_t ps = v.read_ps[r];
		const int32_t hp = v.read_hp[r];
		if (hp < 0 || ps < 0) continue;
		if (hp > 1) {
			++p.n_skipped;
			continue;
		}
		auto it = ps_id.find(ps);
		if (it == ps_id.end()) {
			if (p.phaseset.size() >= TP_MAX_PHASESETS - 1) {
				msg = "2^30 or more phase sets in one problem";
				return WHAMD_ERR_UNSUPPORTED;
			}
			it = ps_id.emplace(ps, (uint32_t)p.phaseset.size()).first;
			p.phaseset.push_back(ps);
		}
		p.read_code[r] = it->second << 1 | (uint32_t)hp;
	}

	// entries: bounds of each, the voting ones counted and their magnitudes summed
	const uint32_t n_threads = host_threads(n_entries + n_reads, 1 << 16);
	std::vector<uint64_t> bad(n_threads, NONE), voting(n_threads, 0), magnitude(n_threads, 0);
	parallel_ranges(n_reads, n_threads, [&](uint64_t b, uint64_t e, uint32_t t) {
		uint64_t my_bad = NONE, my_voting = 0, my_magnitude = 0;   // (the threads' slots share cache lines: one write each at the end)
		for (uint64_t r = b; r < e; r++) {
			const bool counted = p.read_code[r] != TP_NOT_COUNTED;
			for (uint64_t x = v.read_ptr[r]; x < v.read_ptr[r + 1]; x++) {
				if (v.entry_variant[x] >= n_var || v.entry_id[x] > 1) {
					if (my_bad == NONE) my_bad = x;
					continue;
				}
				if (!counted || (v.variant_flags[v.entry_variant[x]] & WHAMD_TAGPHASE_HOMOZYGOUS)) continue;
				++my_voting;
				const int64_t q = v.entry_quality[x];
				my_magnitude += (uint64_t)(q < 0 ? -q : q);
			}
		}
		bad[t] = std::min(bad[t], my_bad);
		voting[t] += my_voting;
		magnitude[t] += my_magnitude;
	});
	uint64_t first_bad = NONE, total_magnitude = 0;
	for (uint32_t t = 0; t < n_threads; t++) {
		first_bad = std::min(first_bad, bad[t]);
		p.n_voting += voting[t];
		total_magnitude += magnitude[t];   // (below 2^32 entries of at most 2^31 each: no wrap)
	}
	if (first_bad != NONE) {
		const uint64_t r = std::upper_bound(v.read_ptr, v.read_ptr + n_reads + 1, first_bad) - v.read_ptr - 1;
		if (v.entry_variant[first_bad] >= n_var)
			msg = "read " + std::to_string(r) + ": variant index " + std::to_string(v.entry_variant[first_bad]) + " out of range (" + std::to_string(n_var) + " variants)";
		else
			msg = "read " + std::to_string(r) + ": id " + std::to_string((int)v.entry_id[first_bad]) + " outside {0, 1}";
		return WHAMD_ERR_INVALID;
	}
	if (total_magnitude > (uint64_t)TP_MAX_MAGNITUDE) {
		msg = "the qualities of the voting entries sum to more than 2^53 in magnitude: score / total would no longer be exact";
		return WHAMD_ERR_UNSUPPORTED;
	}
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- host twin (debug library)
#ifdef WHAMD_DEBUG_BUILD
namespace {

void tagphase_host(const TagphaseProblem& p, TagphaseScores& out) {
	const whamd_tagphase_view& v = *p.view;
	struct Row { uint32_t ps, first; int64_t sums[2]; };
	std::vector<std::vector<Row>> votes(p.n_variants);
	out.count.assign(p.n_variants, 0);
	for (uint64_t r = 0; r < p.n_reads; r++) {
		const uint32_t code = p.read_code[r];
		if (code == TP_NOT_COUNTED) continue;
		for (uint64_t x = v.read_ptr[r]; x < v.read_ptr[r + 1]; x++) {
			const uint32_t var = v.entry_variant[x];
			if (v.variant_flags[var] & WHAMD_TAGPHASE_HOMOZYGOUS) continue;
			std::vector<Row>& rows = votes[var];
			size_t s = 0;
			while (s < rows.size() && rows[s].ps != code >> 1) s++;
			if (s == rows.size()) rows.push_back(Row{code >> 1, (uint32_t)x, {0, 0}});
			rows[s].sums[(code & 1u) ^ v.entry_id[x]] += (int64_t)v.entry_quality[x];
			++out.count[var];
		}
	}
	out.out.resize(p.n_variants);
	out.row_ptr.assign(p.want_table ? p.n_variants + 1 : 0, 0);
	const uint32_t problem_bits = v.only_indels ? (uint32_t)TP_ONLY_INDELS : 0u;
	for (uint64_t x = 0; x < p.n_variants; x++) {
		TpBest best = tp_start();
		for (const Row& row : votes[x]) tp_consider(best, row.sums[0], row.sums[1], row.ps, row.first);
		out.out[x] = tp_result(best, v.variant_flags[x] | problem_bits, v.gap_threshold);
		if (p.want_table) {
			std::vector<Row> by_id(votes[x]);
			std::sort(by_id.begin(), by_id.end(), [](const Row& a, const Row& b) { return a.ps < b.ps; });   // (the device's order)
			for (const Row& row : by_id) out.rows.push_back(TpRow{row.sums[0], row.sums[1], row.ps, row.first, {0, 0}});
			out.row_ptr[x + 1] = out.rows.size();
		}
	}
}

}  // namespace
#endif

// ---------------------------------------------------------------------------------------------- C ABI
struct whamd_tagphase_result {
	struct Problem {
		std::vector<uint8_t> voted, best_id, kept, zero_total;
		std::vector<uint64_t> first;
		std::vector<uint32_t> n_phasesets;
		std::vector<int64_t> best_ps, score, total;
		std::vector<uint64_t> row_ptr, row_first;
		std::vector<int64_t> row_ps, row_sum0, row_sum1;
		whamd_tagphase_stats stats{};
	};
	std::vector<Problem> problems;
};

namespace {

void assemble(const TagphaseProblem& p, const TagphaseScores& sc, whamd_tagphase_result::Problem& out) {
	const uint64_t n = p.n_variants;
	out.voted.assign(n, 0);
	out.best_id.assign(n, 0);
	out.kept.assign(n, 0);
	out.zero_total.assign(n, 0);
	out.first.assign(n, NONE);
	out.n_phasesets.assign(n, 0);
	out.best_ps.assign(n, 0);
	out.score.assign(n, 0);
	out.total.assign(n, 0);
	whamd_tagphase_stats& s = out.stats;
	s.n_reads = p.n_reads;
	s.n_variants = n;
	s.n_entries = p.n_entries;
	s.n_voting = p.n_voting;
	s.n_skipped = p.n_skipped;
	if (p.want_table) out.row_ptr.assign(n + 1, 0);
	if (sc.out.empty()) return;   // (nothing voted)
	for (uint64_t x = 0; x < n; x++) {
		const TpOut& o = sc.out[x];
		if (!(o.flags & TP_VOTED)) continue;
		out.voted[x] = 1;
		out.best_id[x] = o.flags & TP_BEST_ID ? 1 : 0;
		out.kept[x] = o.flags & TP_KEPT ? 1 : 0;
		out.zero_total[x] = o.flags & TP_ZERO_TOTAL ? 1 : 0;
		out.first[x] = o.first;
		out.n_phasesets[x] = o.n_ps;
		out.best_ps[x] = p.phaseset[o.best_ps];
		out.score[x] = o.score;
		out.total[x] = o.total;
		++s.n_voted;
		s.n_kept += out.kept[x];
		s.n_zero_total += out.zero_total[x];
		const uint32_t c = sc.count[x];
		++(c <= TP_CLASS_A_MAX ? s.variants_class_a : c <= TP_CLASS_B_MAX ? s.variants_class_b : s.variants_class_c);
		if (o.n_ps > TP_REG_PHASESETS) ++s.variants_many_phase_sets;
	}
	if (!p.want_table || sc.row_ptr.empty()) return;
	const uint64_t n_rows = sc.rows.size();
	out.row_ptr.assign(sc.row_ptr.begin(), sc.row_ptr.end());
	out.row_first.resize(n_rows);
	out.row_ps.resize(n_rows);
	out.row_sum0.resize(n_rows);
	out.row_sum1.resize(n_rows);
	std::vector<TpRow> rows;
	for (uint64_t x = 0; x < n; x++) {
		rows.assign(sc.rows.begin() + sc.row_ptr[x], sc.rows.begin() + sc.row_ptr[x + 1]);
		std::sort(rows.begin(), rows.end(), [](const TpRow& a, const TpRow& b) { return a.first < b.first; });
		for (size_t k = 0; k < rows.size(); k++) {
			const uint64_t at = sc.row_ptr[x] + k;
			out.row_first[at] = rows[k].first;
			out.row_ps[at] = p.phaseset[rows[k].ps];
			out.row_sum0[at] = rows[k].sum0;
			out.row_sum1[at] = rows[k].sum1;
		}
	}
	s.table_rows = n_rows;
}

whamd_status_t tagphase(const whamd_tagphase_view* views, uint64_t n, int device, bool host, whamd_tagphase_result** out) {
	return run_batch<TagphaseProblem, TagphaseScores>(
		views, n, host, out, tagphase_prepare,
		[](auto& problems, auto& scores) {
			for (size_t x = 0; x < problems.size(); x++)
				if (problems[x].n_voting) tagphase_host(problems[x], scores[x]);
		},
		[&](auto& problems, auto& scores, CallTimes& times, std::string& msg) { return tagphase_device(problems, device, scores, times, msg); }, assemble);
}

}  // namespace

extern "C" {

whamd_status_t whamd_tagphase(const whamd_tagphase_view* problems, uint64_t n_problems, int device, whamd_tagphase_result** out) {
	return guarded([&]() -> whamd_status_t { return tagphase(problems, n_problems, device, false, out); });
}

uint64_t whamd_tagphase_problem_count(const whamd_tagphase_result* r) { return r ? r->problems.size() : 0; }

uint64_t whamd_tagphase_count(const whamd_tagphase_result* r, uint64_t m) { return r && m < r->problems.size() ? r->problems[m].voted.size() : 0; }

whamd_status_t whamd_tagphase_get(const whamd_tagphase_result* r, uint64_t m, uint8_t* voted_out, uint64_t* first_out, uint32_t* n_phasesets_out,
                                  int64_t* best_ps_out, uint8_t* best_id_out, int64_t* score_out, int64_t* total_out, uint8_t* kept_out,
                                  uint8_t* zero_total_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	copy_out(voted_out, p->voted);
	copy_out(first_out, p->first);
	copy_out(n_phasesets_out, p->n_phasesets);
	copy_out(best_ps_out, p->best_ps);
	copy_out(best_id_out, p->best_id);
	copy_out(score_out, p->score);
	copy_out(total_out, p->total);
	copy_out(kept_out, p->kept);
	copy_out(zero_total_out, p->zero_total);
	return WHAMD_OK;
}

uint64_t whamd_tagphase_row_count(const whamd_tagphase_result* r, uint64_t m) { return r && m < r->problems.size() ? r->problems[m].row_ps.size() : 0; }

whamd_status_t whamd_tagphase_get_table(const whamd_tagphase_result* r, uint64_t m, uint64_t* row_ptr_out, int64_t* ps_out, int64_t* sum0_out,
                                        int64_t* sum1_out, uint64_t* first_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	if (p->row_ptr.empty()) return fail(WHAMD_ERR_INVALID, "the problem was not given want_table");
	copy_out(row_ptr_out, p->row_ptr);
	copy_out(ps_out, p->row_ps);
	copy_out(sum0_out, p->row_sum0);
	copy_out(sum1_out, p->row_sum1);
	copy_out(first_out, p->row_first);
	return WHAMD_OK;
}

whamd_status_t whamd_tagphase_get_stats(const whamd_tagphase_result* r, uint64_t m, whamd_tagphase_stats* stats_out) {
	return get_stats_of(r, m, stats_out);
}

void whamd_tagphase_destroy(whamd_tagphase_result* r) { delete r; }

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_tagphase_host(const whamd_tagphase_view* problems, uint64_t n_problems, whamd_tagphase_result** out) {
	return guarded([&]() -> whamd_status_t { return tagphase(problems, n_problems, 0, true, out); });
}
#endif

}  // extern "C"
