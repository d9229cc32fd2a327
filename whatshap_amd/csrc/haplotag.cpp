// haplotag.cpp -- the host side of haplotagging (haplotag.h): validation, phase sets to dense ids and phasings to haplotype masks, the
// sequential grouping of reads, result assembly, the C ABI of whatshap_amd.h's haplotag section; and, in the debug library only, the
// one-thread host twin of the scoring (whamd_debug_haplotag_host).
#include "haplotag.h"

#include <algorithm>
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

HtBounds g_bounds{HT_CLASS_A_MAX, HT_CLASS_B_MAX};

void refresh_bounds() {
#ifdef WHAMD_DEBUG_BUILD
	const char* a = getenv("WHAMD_HT_CLASS_A_MAX");
	const char* b = getenv("WHAMD_HT_CLASS_B_MAX");
	g_bounds.a_max = a && atoll(a) > 0 ? (uint32_t)atoll(a) : HT_CLASS_A_MAX;
	g_bounds.b_max = std::max<uint32_t>(g_bounds.a_max, b && atoll(b) > 0 ? (uint32_t)atoll(b) : HT_CLASS_B_MAX);
#endif
}

}  // namespace

const HtBounds& whamd::haplotag_bounds() { return g_bounds; }

// ---------------------------------------------------------------------------------------------- validation, variants, groups
whamd_status_t whamd::haplotag_prepare(const whamd_haplotag_view& v, HaplotagProblem& p, std::string& msg) {
	if (v.ploidy < 2) {
		msg = "ploidy " + std::to_string(v.ploidy) + " below 2: there is no second-best haplotype (the reference raises IndexError)";
		return WHAMD_ERR_INVALID;
	}
	if (v.ploidy > HT_MAX_PLOIDY) {
		msg = "ploidy " + std::to_string(v.ploidy) + " above the limit of " + std::to_string(HT_MAX_PLOIDY);
		return WHAMD_ERR_INVALID;
	}
	if (v.n_reads && (!v.read_ptr || !v.read_start || !v.read_repr)) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (v.n_variants && (!v.variant_position || !v.variant_phaseset || !v.variant_phasing)) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (v.n_reads >= 0xffffffffull || v.n_variants >= 0x80000000ull) {
		msg = "more than 2^32 - 2 reads or 2^31 - 1 variants in one problem";
		return WHAMD_ERR_UNSUPPORTED;
	}
	const uint64_t n_reads = v.n_reads, n_entries = n_reads ? v.read_ptr[n_reads] : 0;
	if (!check_offsets(v.read_ptr, n_reads, "read_ptr", "read", msg)) return WHAMD_ERR_INVALID;
	for (uint64_t r = 0; r < n_reads; r++)
		if (v.read_repr[r] >= n_reads || (v.read_bx && v.read_bx[r] != HT_NO_BX && v.read_bx[r] >= n_reads)) {
			msg = "read " + std::to_string(r) + ": representation and BX ids must be dense (below the number of reads)";
			return WHAMD_ERR_INVALID;
		}
	if (n_entries && (!v.entry_position || !v.entry_allele || !v.entry_quality)) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	p.ploidy = v.ploidy;
	p.n_reads = n_reads;
	p.read_ptr = v.read_ptr;
	p.quality = v.entry_quality;
	p.read_start = v.read_start;

	// variants: position order for the lookup, phase sets to dense ids in table order, phasings to masks
	const uint32_t n_var = (uint32_t)v.n_variants;
	std::vector<std::pair<int64_t, uint32_t>> by_pos(n_var);
	for (uint32_t x = 0; x < n_var; x++) by_pos[x] = {v.variant_position[x], x};
	std::sort(by_pos.begin(), by_pos.end());
	for (uint32_t x = 1; x < n_var; x++)
		if (by_pos[x].first == by_pos[x - 1].first) {
			msg = "variant position " + std::to_string(by_pos[x].first) + " is listed twice";
			return WHAMD_ERR_INVALID;
		}
	p.variants.resize(n_var);
	std::unordered_map<int64_t, uint32_t> ps_id;
	for (uint32_t x = 0; x < n_var; x++) {
		auto it = ps_id.find(v.variant_phaseset[x]);
		if (it == ps_id.end()) {
			it = ps_id.emplace(v.variant_phaseset[x], (uint32_t)p.phaseset.size()).first;
			p.phaseset.push_back(v.variant_phaseset[x]);
		}
		uint32_t masks = 0;
		for (uint32_t h = 0; h < v.ploidy; h++) {
			const int8_t a = v.variant_phasing[(uint64_t)x * v.ploidy + h];
			if (a == 1) masks |= 1u << h;
			else if (a == 0) masks |= 1u << (16 + h);
		}
		p.variants[x] = HtVariant{it->second, masks};
	}
	if (p.phaseset.size() >= HT_MAX_PHASESETS) {
		msg = "more than 2^27 - 1 phase sets in one problem";
		return WHAMD_ERR_UNSUPPORTED;
	}

	// entries: the variant each names, the allele in bit 31
	p.entry_var.resize(n_entries);
	const uint32_t n_threads = host_threads(n_entries, 1 << 16);
	std::vector<uint64_t> bad(n_threads, NONE);
	parallel_ranges(n_entries, n_threads, [&](uint64_t b, uint64_t e, uint32_t t) {
		auto it = by_pos.end();
		for (uint64_t x = b; x < e; x++) {
			const int8_t a = v.entry_allele[x];
			// a read lists its variants in position order, mostly without gaps: the next variant of the table first, then the search
			if (it != by_pos.end() && ++it != by_pos.end() && it->first == v.entry_position[x]) {
			} else {
				it = std::lower_bound(by_pos.begin(), by_pos.end(), std::make_pair(v.entry_position[x], (uint32_t)0));
			}
			if ((a != 0 && a != 1) || it == by_pos.end() || it->first != v.entry_position[x]) {
				if (bad[t] == NONE) bad[t] = x;
				p.entry_var[x] = 0;
				continue;
			}
			p.entry_var[x] = it->second | ((uint32_t)a << 31);
		}
	});
	uint64_t first_bad = NONE;
	for (uint64_t b : bad) first_bad = std::min(first_bad, b);
	if (first_bad != NONE) {
		const uint64_t r = std::upper_bound(v.read_ptr, v.read_ptr + n_reads + 1, first_bad) - v.read_ptr - 1;
		const int8_t a = v.entry_allele[first_bad];
		if (a != 0 && a != 1) msg = "read " + std::to_string(r) + ": allele " + std::to_string((int)a) + " outside {0, 1} at position " + std::to_string(v.entry_position[first_bad]);
		else msg = "read " + std::to_string(r) + ": position " + std::to_string(v.entry_position[first_bad]) + " is not in the variant table (unknown position)";
		return WHAMD_ERR_INVALID;
	}

	// the reads of every BX tag in read-set order
	const bool linked = v.linked_reads && v.read_bx;
	std::vector<uint64_t> bx_ptr;
	RawVec<uint32_t> bx_reads;
	if (linked) {
		bx_ptr.assign(n_reads + 1, 0);
		for (uint64_t r = 0; r < n_reads; r++)
			if (v.read_bx[r] != HT_NO_BX) ++bx_ptr[v.read_bx[r] + 1];
		for (uint64_t x = 0; x < n_reads; x++) bx_ptr[x + 1] += bx_ptr[x];
		bx_reads.resize(bx_ptr[n_reads]);
		std::vector<uint64_t> cursor(bx_ptr.begin(), bx_ptr.end() - 1);
		for (uint64_t r = 0; r < n_reads; r++)
			if (v.read_bx[r] != HT_NO_BX) bx_reads[cursor[v.read_bx[r]]++] = (uint32_t)r;
	}
	// the groups, in read order
	std::vector<uint8_t> processed(n_reads, 0);   // by representation id
	p.group_ptr.assign(1, 0);
	p.members.reserve(n_reads);
	for (uint64_t r = 0; r < n_reads; r++) {
		if (processed[v.read_repr[r]]) continue;
		processed[v.read_repr[r]] = 1;
		const size_t begin = p.members.size();
		p.members.push_back((uint32_t)r);
		const bool with_bx = linked && v.read_bx[r] != HT_NO_BX;
		if (with_bx && v.linked_read_cutoff >= 0) {
			const uint32_t bx = v.read_bx[r];
			const int64_t start = v.read_start[r];
			for (uint64_t x = bx_ptr[bx]; x < bx_ptr[bx + 1]; x++) {
				const uint32_t o = bx_reads[x];
				if (processed[v.read_repr[o]]) continue;   // (the seed itself, and every read that shares its representation)
				const int64_t so = v.read_start[o];
				const uint64_t dist = start > so ? (uint64_t)start - (uint64_t)so : (uint64_t)so - (uint64_t)start;
				if (dist <= (uint64_t)v.linked_read_cutoff) p.members.push_back(o);
			}
		}
		uint64_t entries = 0;
		for (size_t x = begin; x < p.members.size(); x++) {
			const uint32_t o = p.members[x];
			processed[v.read_repr[o]] = 1;
			entries += v.read_ptr[o + 1] - v.read_ptr[o];
		}
		if (entries >= 0x80000000ull) {
			msg = "a group of reads lists more than 2^31 - 1 variants";
			return WHAMD_ERR_UNSUPPORTED;
		}
		p.group_ptr.push_back(p.members.size());
		p.group_bx.push_back(with_bx ? v.read_bx[r] : HT_NO_BX);
		p.group_entries.push_back(entries);
		p.n_entries += entries;
	}
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- host twin (debug library)
#ifdef WHAMD_DEBUG_BUILD
namespace {

struct PsSums {
	int64_t sums[HT_MAX_PLOIDY];
	uint32_t ps, first;
};

void haplotag_score_host(const HaplotagProblem& p, HaplotagScores& out) {
	const uint64_t n_groups = p.n_groups();
	out.out.resize(n_groups);
	std::vector<PsSums> found;
	std::unordered_map<uint32_t, uint32_t> slot_of;   // used once a group has many phase sets
	for (uint64_t g = 0; g < n_groups; g++) {
		found.clear();
		slot_of.clear();
		uint32_t index = 0;
		for (uint64_t m = p.group_ptr[g]; m < p.group_ptr[g + 1]; m++) {
			const uint32_t r = p.members[m];
			for (uint64_t x = p.read_ptr[r]; x < p.read_ptr[r + 1]; x++, index++) {
				const HtVariant& var = p.variants[p.entry_var[x] & 0x7fffffffu];
				const uint32_t match = ht_match(p.entry_var[x], var.masks);
				if (!match) continue;
				uint32_t s = (uint32_t)found.size();
				if (found.size() <= 16) {
					for (uint32_t y = 0; y < found.size(); y++)
						if (found[y].ps == var.ps) s = y;
				} else {
					const auto it = slot_of.find(var.ps);
					if (it != slot_of.end()) s = it->second;
				}
				if (s == found.size()) {
					PsSums fresh{};
					fresh.ps = var.ps;
					fresh.first = index;
					found.push_back(fresh);
					if (found.size() == 17)
						for (uint32_t y = 0; y < 17; y++) slot_of[found[y].ps] = y;
					else if (found.size() > 17) slot_of[var.ps] = s;
				}
				for (uint32_t h = 0; h < p.ploidy; h++)
					if (match >> h & 1) found[s].sums[h] = (int64_t)((uint64_t)found[s].sums[h] + (uint64_t)(int64_t)p.quality[x]);
			}
		}
		HtBest best{};
		for (const PsSums& f : found) ht_consider<(int)HT_MAX_PLOIDY>(best, f.sums, p.ploidy, f.ps, f.first);
		out.out[g] = ht_result(best, (uint32_t)found.size());
	}
}

}  // namespace
#endif

// ---------------------------------------------------------------------------------------------- C ABI
struct whamd_haplotag_result {
	struct Problem {
		RawVec<int32_t> haplotype;      // per read
		RawVec<int64_t> quality, phaseset;
		std::vector<uint32_t> bx;       // the assigned linked-read groups in processing order
		std::vector<int64_t> bx_start, bx_phaseset;
		std::vector<int32_t> bx_haplotype;
		whamd_haplotag_stats stats{};
	};
	std::vector<Problem> problems;
};

namespace {

void assemble(const HaplotagProblem& p, const HaplotagScores& sc, whamd_haplotag_result::Problem& out) {
	out.haplotype.assign(p.n_reads, -1);
	out.quality.assign(p.n_reads, 0);
	out.phaseset.assign(p.n_reads, 0);
	whamd_haplotag_stats& s = out.stats;
	s.n_reads = p.n_reads;
	s.n_groups = p.n_groups();
	s.n_entries = p.n_entries;
	for (uint64_t g = 0; g < p.n_groups(); g++) {
		if (!p.group_entries[g]) continue;
		const HtOut& o = sc.out[g];
		const uint32_t n_ps = o.hap_nps >> 5, hap1 = o.hap_nps & 31u;
		const uint32_t cls = haplotag_class_of(p.group_entries[g]);
		++(cls == 0 ? s.groups_class_a : cls == 1 ? s.groups_class_b : s.groups_class_c);
		if (n_ps > HT_REG_PHASESETS) ++s.groups_many_phase_sets;
		if (n_ps > 1) ++s.n_multiple_phase_sets;
		if (!hap1) continue;
		++s.n_assigned;
		const int64_t phaseset = p.phaseset[o.ps];
		for (uint64_t m = p.group_ptr[g]; m < p.group_ptr[g + 1]; m++) {
			const uint32_t r = p.members[m];
			out.haplotype[r] = (int32_t)hap1 - 1;
			out.quality[r] = o.quality;
			out.phaseset[r] = phaseset;
		}
		if (p.group_bx[g] != HT_NO_BX) {
			out.bx.push_back(p.group_bx[g]);
			out.bx_start.push_back(p.read_start[p.members[p.group_ptr[g]]]);
			out.bx_haplotype.push_back((int32_t)hap1 - 1);
			out.bx_phaseset.push_back(phaseset);
		}
	}
}

whamd_status_t haplotag(const whamd_haplotag_view* views, uint64_t n, int device, bool host, whamd_haplotag_result** out) {
	return run_batch<HaplotagProblem, HaplotagScores>(
		views, n, host, out,
		[](const whamd_haplotag_view& v, HaplotagProblem& p, std::string& msg) {
			refresh_bounds();   // (the debug library's class bounds may change between calls)
			return haplotag_prepare(v, p, msg);
		},
		[](auto& problems, auto& scores) {
			for (size_t x = 0; x < problems.size(); x++) haplotag_score_host(problems[x], scores[x]);
		},
		[&](auto& problems, auto& scores, CallTimes& times, std::string& msg) { return haplotag_score_device(problems, device, scores, times, msg); }, assemble);
}

}  // namespace

extern "C" {

whamd_status_t whamd_haplotag(const whamd_haplotag_view* problems, uint64_t n_problems, int device, whamd_haplotag_result** out) {
	return guarded([&]() -> whamd_status_t { return haplotag(problems, n_problems, device, false, out); });
}

uint64_t whamd_haplotag_problem_count(const whamd_haplotag_result* r) { return r ? r->problems.size() : 0; }

uint64_t whamd_haplotag_count(const whamd_haplotag_result* r, uint64_t m) { return r && m < r->problems.size() ? r->problems[m].haplotype.size() : 0; }

whamd_status_t whamd_haplotag_get(const whamd_haplotag_result* r, uint64_t m, int32_t* haplotype_out, int64_t* quality_out, int64_t* phaseset_out) {
	const auto* found = problem_of(r, m);
	if (!found) return no_problem(r);
	const whamd_haplotag_result::Problem& p = *found;
	const size_t n = p.haplotype.size();
	if (haplotype_out && n) std::memcpy(haplotype_out, p.haplotype.data(), n * 4);
	if (quality_out && n) std::memcpy(quality_out, p.quality.data(), n * 8);
	if (phaseset_out && n) std::memcpy(phaseset_out, p.phaseset.data(), n * 8);
	return WHAMD_OK;
}

uint64_t whamd_haplotag_bx_count(const whamd_haplotag_result* r, uint64_t m) { return r && m < r->problems.size() ? r->problems[m].bx.size() : 0; }

whamd_status_t whamd_haplotag_get_bx(const whamd_haplotag_result* r, uint64_t m, uint32_t* bx_out, int64_t* reference_start_out, int32_t* haplotype_out,
                                     int64_t* phaseset_out) {
	const auto* found = problem_of(r, m);
	if (!found) return no_problem(r);
	const whamd_haplotag_result::Problem& p = *found;
	const size_t n = p.bx.size();
	if (bx_out && n) std::memcpy(bx_out, p.bx.data(), n * 4);
	if (reference_start_out && n) std::memcpy(reference_start_out, p.bx_start.data(), n * 8);
	if (haplotype_out && n) std::memcpy(haplotype_out, p.bx_haplotype.data(), n * 4);
	if (phaseset_out && n) std::memcpy(phaseset_out, p.bx_phaseset.data(), n * 8);
	return WHAMD_OK;
}

whamd_status_t whamd_haplotag_get_stats(const whamd_haplotag_result* r, uint64_t m, whamd_haplotag_stats* stats_out) {
	return get_stats_of(r, m, stats_out);
}

void whamd_haplotag_destroy(whamd_haplotag_result* r) { delete r; }

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_haplotag_host(const whamd_haplotag_view* problems, uint64_t n_problems, whamd_haplotag_result** out) {
	return guarded([&]() -> whamd_status_t { return haplotag(problems, n_problems, 0, true, out); });
}
#endif

}  // extern "C"
