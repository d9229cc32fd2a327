// readmerge.cpp -- the host side of the read merging (readmerge.h): validation, the reads' begin / len / packed alleles and partner
// ranges, the union-find over the blue edges, the member lists of the merged components, result assembly, the C ABI of whatshap_amd.h's read
// merging section; and, in the debug library only, the one-thread host twin of both device stages (whamd_debug_readmerge_host).
#include "readmerge.h"

#include <algorithm>
#include <limits>

#include "../../include/whatshap_amd_debug.h"
#include "batch_call.h"
#include "debug_build.h"

using namespace whamd;

// ---------------------------------------------------------------------------------------------- validation, packing, partner ranges
whamd_status_t whamd::readmerge_prepare(const whamd_readmerge_view& v, ReadmergeProblem& p, std::string& msg) {
	if (v.n_reads && !v.read_ptr) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (v.n_reads >= RM_MAX_COUNT) {
		msg = "2^32 - 4096 or more reads in one problem";
		return WHAMD_ERR_UNSUPPORTED;
	}
	const uint64_t n = v.n_reads;
	if (!check_offsets(v.read_ptr, n, "read_ptr", "read", msg)) return WHAMD_ERR_INVALID;
	const uint64_t n_entries = n ? v.read_ptr[n] : 0;
	if (n_entries && (!v.entry_position || !v.entry_allele || !v.entry_quality)) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (n_entries >= RM_MAX_COUNT) {
		msg = "2^32 - 4096 or more entries in one problem";
		return WHAMD_ERR_UNSUPPORTED;
	}
	for (uint64_t r = 0; r < n; r++)
		if (v.read_ptr[r] == v.read_ptr[r + 1]) {
			msg = "read " + std::to_string(r) + " has no variants";
			return WHAMD_ERR_INVALID;
		}
	uint64_t magnitude = 0;
	bool too_large = false;
	for (uint64_t x = 0; x < n_entries; x++) {
		if (v.entry_allele[x] > 1) {
			const uint64_t r = std::upper_bound(v.read_ptr, v.read_ptr + n + 1, x) - v.read_ptr - 1;
			msg = "read " + std::to_string(r) + ": allele " + std::to_string((int)v.entry_allele[x]) + " outside {0, 1}";
			return WHAMD_ERR_INVALID;
		}
		const int64_t pos = v.entry_position[x];
		if (pos >= RM_MAX_POSITION || pos < -RM_MAX_POSITION) {
			msg = "a position of magnitude 2^62 or more: begin + len and the hang of a pair would leave int64";
			return WHAMD_ERR_UNSUPPORTED;
		}
		const int64_t q = v.entry_quality[x];
		const uint64_t a = q < 0 ? (uint64_t)0 - (uint64_t)q : (uint64_t)q;
		too_large = too_large || __builtin_add_overflow(magnitude, a, &magnitude);
	}
	if (too_large || magnitude > (uint64_t)std::numeric_limits<int64_t>::max()) {
		msg = "the qualities sum to more than 2^63 - 1 in magnitude: a superread's sums could leave int64";
		return WHAMD_ERR_UNSUPPORTED;
	}
	p.view = &v;
	p.n_reads = n;
	p.n_entries = n_entries;
	p.want_edges = v.want_edges != 0;
	p.thr = RmThresholds{v.thr_diff, v.thr_neg_diff, v.max_error_rate};
	p.given = v.representative != nullptr;
	if (p.given) {
		// smallest id as representative: rep[i] <= i and rep[rep[i]] == rep[i]
		for (uint64_t r = 0; r < n; r++) {
			const uint32_t rep = v.representative[r];
			if (rep > r || v.representative[rep] != rep) {
				msg = "read " + std::to_string(r) + ": representative " + std::to_string(rep) + " is not the smallest id of a component";
				return WHAMD_ERR_INVALID;
			}
		}
		return WHAMD_OK;
	}
	p.reads.resize(n);
	uint64_t n_words = 0;
	for (uint64_t r = 0; r < n; r++) {
		const uint64_t len = v.read_ptr[r + 1] - v.read_ptr[r];
		p.reads[r] = RmRead{v.entry_position[v.read_ptr[r]], (uint32_t)len, (uint32_t)n_words};
		n_words += (len + 63) >> 6;
	}
	p.n_words = n_words;   // (at most n_entries: every read has an entry)
	p.words.assign(n_words, 0);
	for (uint64_t r = 0; r < n; r++) {
		uint64_t* w = p.words.data() + p.reads[r].word;
		const uint8_t* a = v.entry_allele + v.read_ptr[r];
		for (uint32_t t = 0; t < p.reads[r].len; t++) w[t >> 6] |= (uint64_t)a[t] << (t & 63u);
	}
	// hi_j + 1: the first t > j with begin_t >= end_j
	bool sorted = true;
	for (uint64_t r = 1; r < n && sorted; r++) sorted = p.reads[r - 1].begin <= p.reads[r].begin;
	std::vector<int64_t> begins;
	if (sorted) {
		begins.resize(n);
		for (uint64_t r = 0; r < n; r++) begins[r] = p.reads[r].begin;
	}
	p.pair_ptr.assign(n + 1, 0);
	for (uint64_t j = 0; j < n; j++) {
		const int64_t end = p.reads[j].begin + (int64_t)p.reads[j].len;
		uint64_t t;
		if (sorted) {
			t = std::lower_bound(begins.begin() + j + 1, begins.end(), end) - begins.begin();
		} else {
			t = j + 1;
			while (t < n && p.reads[t].begin < end) t++;
		}
		p.pair_ptr[j + 1] = p.pair_ptr[j] + (t - j - 1);
		if (p.pair_ptr[j + 1] >= RM_MAX_COUNT) {
			msg = "2^32 - 4096 or more pairs of reads to compare in one problem";
			return WHAMD_ERR_UNSUPPORTED;
		}
	}
	p.n_pairs = p.pair_ptr[n];
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- components, slots
void whamd::readmerge_components(const ReadmergeProblem& p, ReadmergeScores& sc) {
	const whamd_readmerge_view& v = *p.view;
	const uint64_t n = p.n_reads;
	sc.representative.resize(n);
	if (p.given) {
		std::copy(v.representative, v.representative + n, sc.representative.begin());
	} else {
		std::vector<uint32_t>& parent = sc.representative;
		for (uint64_t r = 0; r < n; r++) parent[r] = (uint32_t)r;
		const auto find = [&](uint32_t x) {
			uint32_t root = x;
			while (parent[root] != root) root = parent[root];
			while (parent[x] != root) {
				const uint32_t up = parent[x];
				parent[x] = root;
				x = up;
			}
			return root;
		};
		for (const RmEdge& e : sc.edges) {
			const uint32_t a = find(e.j), b = find(e.i);
			if (a != b) parent[std::max(a, b)] = std::min(a, b);   // the smaller root stays: a root is its component's smallest id
			if (e.flags & RM_NOT_BLUE) ++sc.n_not_blue;
		}
		for (uint64_t r = 0; r < n; r++) parent[r] = find((uint32_t)r);
	}
	std::vector<uint32_t> count(n, 0);
	for (uint64_t r = 0; r < n; r++) ++count[sc.representative[r]];
	sc.comp_size.resize(n);
	for (uint64_t r = 0; r < n; r++) sc.comp_size[r] = count[sc.representative[r]];
	// the members of every component of more than one read, ascending (a counting sort by representative)
	std::vector<uint64_t> first(n + 1, 0);
	for (uint64_t r = 0; r < n; r++) first[r + 1] = first[r] + (count[r] > 1 ? count[r] : 0);
	std::vector<uint32_t> members(first[n]), at(n, 0);
	for (uint64_t r = 0; r < n; r++) {
		const uint32_t rep = sc.representative[r];
		if (count[rep] > 1) members[first[rep] + at[rep]++] = (uint32_t)r;
	}
	sc.member_ptr.assign(1, 0);
	for (uint64_t rep = 0; rep < n; rep++) {
		if (count[rep] <= 1 || sc.representative[rep] != rep) continue;
		sc.merged_reps.push_back((uint32_t)rep);
		sc.member_ptr.push_back(first[rep + 1]);
		for (uint64_t m = first[rep]; m < first[rep + 1]; m++) sc.n_merged_entries += v.read_ptr[members[m] + 1] - v.read_ptr[members[m]];
	}
	sc.members = std::move(members);   // (first[] of a merged representative is its member_ptr: only merged components have members)
}

// ---------------------------------------------------------------------------------------------- host twin (debug library)
#ifdef WHAMD_DEBUG_BUILD
namespace {

void readmerge_pairs_host(const ReadmergeProblem& p, ReadmergeScores& sc) {
	if (p.given) return;
	for (uint64_t j = 0; j < p.n_reads; j++)
		for (uint64_t i = j + 1; i <= j + (p.pair_ptr[j + 1] - p.pair_ptr[j]); i++) {
			uint32_t start;
			const uint32_t L = rm_overlap(p.reads[j], p.reads[i], start);
			const uint32_t mismatch = rm_mismatches(p.words.data(), p.reads[j], p.reads[i], start, L);
			const uint32_t flags = rm_flags(L, mismatch, p.thr);
			if (flags) sc.edges.push_back(RmEdge{(uint32_t)j, (uint32_t)i, L - mismatch, mismatch, flags});
		}
}

// The superreads in plain loops: per component the sorted distinct positions of its members, every entry added at its position's place.
void readmerge_sums_host(const ReadmergeProblem& p, ReadmergeScores& sc) {
	const whamd_readmerge_view& v = *p.view;
	sc.super_ptr.assign(p.n_reads + 1, 0);
	std::vector<int64_t> positions;
	size_t c = 0;
	for (uint64_t rep = 0; rep < p.n_reads; rep++) {
		sc.super_ptr[rep + 1] = sc.super_ptr[rep];
		if (c == sc.merged_reps.size() || sc.merged_reps[c] != rep) continue;
		positions.clear();
		for (uint64_t m = sc.member_ptr[c]; m < sc.member_ptr[c + 1]; m++)
			positions.insert(positions.end(), v.entry_position + v.read_ptr[sc.members[m]], v.entry_position + v.read_ptr[sc.members[m] + 1]);
		std::sort(positions.begin(), positions.end());
		positions.erase(std::unique(positions.begin(), positions.end()), positions.end());
		const uint64_t base = sc.slot_position.size();
		sc.slot_position.insert(sc.slot_position.end(), positions.begin(), positions.end());
		sc.super_ptr[rep + 1] = base + positions.size();
		sc.sums.resize(2 * sc.slot_position.size(), 0);
		for (uint64_t m = sc.member_ptr[c]; m < sc.member_ptr[c + 1]; m++)
			for (uint64_t x = v.read_ptr[sc.members[m]]; x < v.read_ptr[sc.members[m] + 1]; x++) {
				const uint64_t slot = base + (std::lower_bound(positions.begin(), positions.end(), v.entry_position[x]) - positions.begin());
				sc.sums[2 * slot + v.entry_allele[x]] += v.entry_quality[x];
			}
		c++;
	}
	const uint64_t n_slots = sc.slot_position.size();
	sc.allele.resize(n_slots);
	sc.quality.resize(n_slots);
	for (uint64_t s = 0; s < n_slots; s++) rm_decide(sc.sums[2 * s], sc.sums[2 * s + 1], sc.allele[s], sc.quality[s]);
}

}  // namespace
#endif

// ---------------------------------------------------------------------------------------------- C ABI
struct whamd_readmerge_result {
	struct Problem {
		std::vector<uint32_t> representative, comp_size;
		std::vector<uint64_t> super_ptr;
		std::vector<int64_t> position, quality, sum0, sum1;
		std::vector<uint8_t> allele;
		bool want_edges = false;
		std::vector<uint32_t> edge_j, edge_i, edge_match, edge_mismatch;
		std::vector<uint8_t> edge_not_blue;
		whamd_readmerge_stats stats{};
	};
	std::vector<Problem> problems;
};

namespace {

void assemble(ReadmergeProblem& p, ReadmergeScores& sc, whamd_readmerge_result::Problem& out) {
	whamd_readmerge_stats& s = out.stats;
	s.n_reads = p.n_reads;
	s.n_entries = p.n_entries;
	s.n_pairs = p.n_pairs;
	s.n_blue = sc.edges.size();
	s.n_not_blue = sc.n_not_blue;
	s.n_merged_components = sc.merged_reps.size();
	s.n_merged_entries = sc.n_merged_entries;
	s.n_super_entries = sc.slot_position.size();
	out.want_edges = p.want_edges;
	if (p.want_edges) {
		const size_t m = sc.edges.size();
		out.edge_j.resize(m);
		out.edge_i.resize(m);
		out.edge_match.resize(m);
		out.edge_mismatch.resize(m);
		out.edge_not_blue.resize(m);
		for (size_t k = 0; k < m; k++) {
			const RmEdge& e = sc.edges[k];
			out.edge_j[k] = e.j;
			out.edge_i[k] = e.i;
			out.edge_match[k] = e.match;
			out.edge_mismatch[k] = e.mismatch;
			out.edge_not_blue[k] = e.flags & RM_NOT_BLUE ? 1 : 0;
		}
	}
	if (sc.super_ptr.empty()) sc.super_ptr.assign(p.n_reads + 1, 0);   // (a host call of the product library computes nothing)
	out.representative = std::move(sc.representative);
	out.comp_size = std::move(sc.comp_size);
	out.super_ptr = std::move(sc.super_ptr);
	out.position = std::move(sc.slot_position);
	out.allele = std::move(sc.allele);
	out.quality = std::move(sc.quality);
	const size_t n_slots = out.position.size();
	out.sum0.resize(n_slots);
	out.sum1.resize(n_slots);
	for (size_t k = 0; k < n_slots && 2 * k + 1 < sc.sums.size(); k++) {
		out.sum0[k] = sc.sums[2 * k];
		out.sum1[k] = sc.sums[2 * k + 1];
	}
}

whamd_status_t readmerge(const whamd_readmerge_view* views, uint64_t n, int device, bool host, whamd_readmerge_result** out) {
	double pair_kernel_ms = 0, components_ms = 0;
	const whamd_status_t st = run_batch<ReadmergeProblem, ReadmergeScores>(
		views, n, host, out, readmerge_prepare,
		[&](auto& problems, auto& scores) {
			for (size_t x = 0; x < problems.size(); x++) {
				readmerge_pairs_host(problems[x], scores[x]);
				const double t0 = now_ms();
				readmerge_components(problems[x], scores[x]);
				components_ms += now_ms() - t0;
				readmerge_sums_host(problems[x], scores[x]);
			}
		},
		[&](auto& problems, auto& scores, CallTimes& times, std::string& msg) {
			CallTimes pairs, sums;
			whamd_status_t st = readmerge_pairs_device(problems, device, scores, pairs, msg);
			if (st != WHAMD_OK) return st;
			const double t0 = now_ms();
			for (size_t x = 0; x < problems.size(); x++) readmerge_components(problems[x], scores[x]);
			components_ms = now_ms() - t0;
			st = readmerge_sums_device(problems, device, scores, sums, msg);
			if (st != WHAMD_OK) return st;
			pair_kernel_ms = pairs.kernel_ms;
			times.launches = pairs.launches + sums.launches;
			times.upload_ms = pairs.upload_ms + sums.upload_ms;
			times.kernel_ms = pairs.kernel_ms + sums.kernel_ms;
			times.download_ms = pairs.download_ms + sums.download_ms;
			return WHAMD_OK;
		},
		assemble);
	if (st != WHAMD_OK) return st;
	for (auto& problem : (*out)->problems) {
		problem.stats.pair_kernel_ms = pair_kernel_ms;
		problem.stats.components_ms = components_ms;
	}
	return WHAMD_OK;
}

}  // namespace

extern "C" {

whamd_status_t whamd_readmerge(const whamd_readmerge_view* problems, uint64_t n_problems, int device, whamd_readmerge_result** out) {
	return guarded([&]() -> whamd_status_t { return readmerge(problems, n_problems, device, false, out); });
}

uint64_t whamd_readmerge_problem_count(const whamd_readmerge_result* r) { return r ? r->problems.size() : 0; }

uint64_t whamd_readmerge_count(const whamd_readmerge_result* r, uint64_t m) { return r && m < r->problems.size() ? r->problems[m].representative.size() : 0; }

uint64_t whamd_readmerge_super_count(const whamd_readmerge_result* r, uint64_t m) { return r && m < r->problems.size() ? r->problems[m].position.size() : 0; }

uint64_t whamd_readmerge_edge_count(const whamd_readmerge_result* r, uint64_t m) { return r && m < r->problems.size() ? r->problems[m].edge_j.size() : 0; }

whamd_status_t whamd_readmerge_get(const whamd_readmerge_result* r, uint64_t m, uint32_t* representative_out, uint32_t* component_size_out,
                                   uint64_t* super_ptr_out, int64_t* position_out, uint8_t* allele_out, int64_t* quality_out, int64_t* sum0_out,
                                   int64_t* sum1_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	copy_out(representative_out, p->representative);
	copy_out(component_size_out, p->comp_size);
	copy_out(super_ptr_out, p->super_ptr);
	copy_out(position_out, p->position);
	copy_out(allele_out, p->allele);
	copy_out(quality_out, p->quality);
	copy_out(sum0_out, p->sum0);
	copy_out(sum1_out, p->sum1);
	return WHAMD_OK;
}

whamd_status_t whamd_readmerge_get_edges(const whamd_readmerge_result* r, uint64_t m, uint32_t* j_out, uint32_t* i_out, uint32_t* match_out,
                                         uint32_t* mismatch_out, uint8_t* not_blue_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	if (!p->want_edges) return fail(WHAMD_ERR_INVALID, "the problem was not given want_edges");
	copy_out(j_out, p->edge_j);
	copy_out(i_out, p->edge_i);
	copy_out(match_out, p->edge_match);
	copy_out(mismatch_out, p->edge_mismatch);
	copy_out(not_blue_out, p->edge_not_blue);
	return WHAMD_OK;
}

whamd_status_t whamd_readmerge_get_stats(const whamd_readmerge_result* r, uint64_t m, whamd_readmerge_stats* stats_out) {
	return get_stats_of(r, m, stats_out);
}

void whamd_readmerge_destroy(whamd_readmerge_result* r) { delete r; }

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_readmerge_host(const whamd_readmerge_view* problems, uint64_t n_problems, whamd_readmerge_result** out) {
	return guarded([&]() -> whamd_status_t { return readmerge(problems, n_problems, 0, true, out); });
}
#endif

}  // extern "C"
